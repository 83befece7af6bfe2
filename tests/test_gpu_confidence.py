"""Matching confidence on the device (include/sgm_mi355x.h, SGM_MatchConfidence; the CONF variants of csrc/sgm_sum_wta.hip)
-- needs an MI355X.

Parity unpinned by the reference (it never exposes min_cost / sec_min_cost): the expected map is the numpy restatement
tests/confidence_ref.py applied to the oracle's aggregated costs (stage 3, digest-pinned to the reference), or to the device's
own S where that is what the contract names (Q14, keep_stages).  The disparity map must be bit-identical to a plain match's.
Tolerance: 0 everywhere -- integers only."""
import json
import os
import subprocess

import numpy as np
import pytest

import confidence_ref as R
from conftest import ROOT, case_inputs, load_npz, option_from_dict
from oracle.pyoracle import default_option, sha

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["cone", "t24x16_d8", "t70x33_d16", "t20x31_d8_tall", "t40x24_d16_dmin3", "t33x33_d12_square", "t64x20_d40",
                "v_default", "v_p1_0_p2_0", "v_p_big", "c1_synth_450x375_d64", "d256_400x48", "d192_300x60"]


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={got[first]} want={want[first]}")


def oracle_aggr(oracle, left, right, opt, honor=False, window=(5, 5)):
    try:
        oracle.set_honor_num_paths(honor)
        oracle.set_census_window(*window)
        return oracle.run(left, right, opt)["aggr"]
    finally:
        oracle.set_honor_num_paths(False)
        oracle.set_census_window(5, 5)


def new_instance(monkeypatch=None, fused=True, batch=1):
    import soc_project_stereo_matching_amd as S
    if monkeypatch is not None:
        monkeypatch.setenv("SGM_FUSED_WTA", "1" if fused else "0")     # read at sgm_create
    return S.SGMInstance(0, batch=batch)


def plain_and_conf(inst, left, right, opt, right_view=False, keep=False):
    """(plain disparity, confidence disparity, confidence) of the same instance state"""
    h, w = left.shape[-2:]
    inst.set_reference_view(right_view)
    inst.keep_stages(keep)
    assert inst.reset(w, h, opt)
    plain = inst.match(left, right)
    assert plain is not None
    assert inst.reset(w, h, opt)
    got = inst.match_confidence(left, right)
    assert got is not None
    return plain, got[0], got[1]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_cases(oracle, golden_cases, monkeypatch, name, fused):
    case = golden_cases[name]
    left, right = case_inputs(case, oracle)
    base = option_from_dict(case["option"])
    S = oracle_aggr(oracle, left, right, base)                        # independent of the view and the uniqueness options
    inst = new_instance(monkeypatch, fused)
    try:
        for right_view in (False, True):
            want = R.confidence(S, base.min_disparity, right_view)[3]
            for unique in (True, False):
                opt = option_from_dict(case["option"])
                opt.is_check_unique = unique
                plain, disp, conf = plain_and_conf(inst, left, right, opt, right_view)
                what = f"{name} fused={fused} right={right_view} unique={unique}"
                assert_same(disp, plain, what + ": disparity")
                assert_same(conf, want, what + ": confidence")
    finally:
        inst.close()


VARIANTS = {
    "d512_separate": dict(w=600, h=20, d=512),
    "d300_dmin5": dict(w=360, h=24, d=300, dmin=5),
    "dmin7_fused": dict(w=160, h=40, d=48, dmin=7),
    "w_lt_h": dict(w=30, h=70, d=16),
    "paths4": dict(w=120, h=48, d=32, honor=True, opt=dict(num_paths=4)),
    "census7x7": dict(w=120, h=48, d=32, window=(7, 7)),
    "census9x7": dict(w=120, h=48, d=32, window=(9, 7)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants(oracle, name):
    v = VARIANTS[name]
    dmin = v.get("dmin", 0)
    left, right = oracle.synth_pair(v["w"], v["h"], v["d"] + dmin, 0xC0F0 + len(name))
    opt = default_option(v["d"] + dmin, dmin, **v.get("opt", {}))
    S = oracle_aggr(oracle, left, right, opt, v.get("honor", False), v.get("window", (5, 5)))
    inst = new_instance()
    try:
        inst.set_honor_num_paths(v.get("honor", False))
        assert inst.set_census_window(*v.get("window", (5, 5)))
        for right_view in (False, True):
            plain, disp, conf = plain_and_conf(inst, left, right, opt, right_view)
            assert_same(disp, plain, f"{name} right={right_view}: disparity")
            assert_same(conf, R.confidence(S, dmin, right_view)[3], f"{name} right={right_view}: confidence")
    finally:
        inst.close()


def test_hole_filling_does_not_change_the_confidence(oracle):
    left, right = oracle.synth_pair(203, 77, 64, 0xC12)
    opt = default_option(64)
    S = oracle_aggr(oracle, left, right, opt)
    inst = new_instance()
    try:
        assert inst.set_fill_holes(True)
        for right_view in (False, True):
            plain, disp, conf = plain_and_conf(inst, left, right, opt, right_view)
            assert not np.isinf(plain).any()
            assert_same(disp, plain, f"fill right={right_view}: disparity")
            assert_same(conf, R.confidence(S, 0, right_view)[3], f"fill right={right_view}: confidence")
    finally:
        inst.close()


@pytest.mark.parametrize("right_view", [False, True], ids=["left", "right"])
def test_keep_stages_and_the_fast_variant_agree(right_view):
    """keep_stages: S stored (the SLOW variant), read back as stage 3 -- the restatement on the device's own S; without it the
    fast variant.  Both give the same map."""
    z = load_npz("cone_inputs.npz")
    opt = default_option(64)
    inst = new_instance()
    try:
        _, disp_k, conf_k = plain_and_conf(inst, z["left"], z["right"], opt, right_view, keep=True)
        S = inst.read_stage("aggr")
        assert_same(conf_k, R.confidence(S, 0, right_view)[3], "keep_stages: confidence vs the device's S")
        _, disp_f, conf_f = plain_and_conf(inst, z["left"], z["right"], opt, right_view, keep=False)
        assert_same(disp_f, disp_k, "disparity with and without keep_stages")
        assert_same(conf_f, conf_k, "confidence with and without keep_stages")
    finally:
        inst.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_q14_match_without_reset(monkeypatch, fused):
    """Two confidence matches without Reset: the second describes the accumulated S (stage 3)."""
    z = load_npz("cone_inputs.npz")
    opt = default_option(64)
    inst = new_instance(monkeypatch, fused)
    try:
        for right_view in (False, True):
            inst.set_reference_view(right_view)
            assert inst.reset(450, 375, opt)
            assert inst.match_confidence(z["left"], z["right"]) is not None
            disp, conf = inst.match_confidence(z["left"], z["right"])
            S = inst.read_stage("aggr")
            assert_same(conf, R.confidence(S, 0, right_view)[3], f"Q14 right={right_view}: confidence vs accumulated S")
            assert inst.reset(450, 375, opt)
            inst.match(z["left"], z["right"])
            plain = inst.match(z["left"], z["right"])
            assert_same(disp, plain, f"Q14 right={right_view}: disparity")
    finally:
        inst.close()


def _kitti_frames():
    with open(os.path.join(ROOT, "tests", "golden", "bench_frames.json")) as f:
        wl = json.load(f)["workloads"]["kitti_1242x375_d128_p8"]
    import soc_project_stereo_matching_amd as S
    seeds = [wl["first_seed"] + k for k in range(8)]
    pairs = [S.synth_pair(wl["w"], wl["h"], wl["d"], s) for s in seeds]
    return wl, seeds, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def test_kitti_batch_of_8_frame_by_frame():
    wl, seeds, left, right = _kitti_frames()
    w, h, d, B = wl["w"], wl["h"], wl["d"], 8
    opt = default_option(d)
    inst, one = new_instance(batch=B), new_instance()
    try:
        assert inst.reset(w, h, opt)
        disp, conf = inst.match_confidence(left, right)
        for f in range(B):
            digests = wl["frames"].get(str(seeds[f]))
            assert one.reset(w, h, opt)                                   # every frame from a zero S (no Q14 accumulation)
            d1, c1 = one.match_confidence(left[f], right[f])
            assert_same(conf[f], c1, f"kitti frame {f}: batch vs alone, confidence")
            assert_same(disp[f], d1, f"kitti frame {f}: batch vs alone, disparity")
            if digests:
                assert sha(disp[f]) == digests["sha256"]["final"], f"kitti frame {f}: reference digest"
        assert (conf > 0).any() and (conf == 0).any()
    finally:
        inst.close()
        one.close()


def test_entry_points_agree():
    """Blocking, async through pageable and pinned buffers, device pointers, SGM_MatchConfidence, and with overlap_post /
    stage CUs on: the same two maps."""
    import torch
    import soc_project_stereo_matching_amd as S
    wl, _, left, right = _kitti_frames()
    w, h, d, B = wl["w"], wl["h"], wl["d"], 2
    left, right = left[:B].copy(), right[:B].copy()
    opt = default_option(d)
    inst = new_instance(batch=B)
    try:
        assert inst.reset(w, h, opt)
        ref_disp, ref_conf = inst.match_confidence(left, right)
        assert_same(ref_disp, inst.match(left, right), "confidence vs plain disparity")
        # async, pageable
        out, conf = np.empty((B, h, w), np.float32), np.empty((B, h, w), np.uint16)
        assert inst.reset(w, h, opt) and inst.match_confidence_async(left, right, out, conf) and inst.match_wait()
        assert_same(out, ref_disp, "async pageable: disparity")
        assert_same(conf, ref_conf, "async pageable: confidence")
        # async, pinned (used in place)
        pl, pr = inst.host_array((B, h, w), np.uint8), inst.host_array((B, h, w), np.uint8)
        po, pc = inst.host_array((B, h, w), np.float32), inst.host_array((B, h, w), np.uint16)
        pl[:], pr[:] = left, right
        for _ in range(2):                                            # back to back: the second waits for the first
            assert inst.reset(w, h, opt) and inst.match_confidence_async(pl, pr, po, pc)
        assert inst.match_wait()
        assert_same(po, ref_disp, "async pinned: disparity")
        assert_same(pc, ref_conf, "async pinned: confidence")
        # device pointers
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        td = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        tc = torch.zeros((B, h, w), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert inst.reset(w, h, opt)
        assert inst.match_confidence_device(tl.data_ptr(), tr.data_ptr(), td.data_ptr(), tc.data_ptr())
        assert inst.synchronize()
        assert_same(td.cpu().numpy(), ref_disp, "device: disparity")
        assert_same(tc.cpu().numpy().view(np.uint16), ref_conf, "device: confidence")
        # NULL conf: false
        assert not inst.lib.sgm_match_confidence(inst.handle, left.ctypes.data, right.ctypes.data, out.ctypes.data, None)
    finally:
        inst.close()
    for setup in ("overlap_post", "stage_cus"):
        inst = new_instance(batch=B)
        try:
            if setup == "overlap_post":
                assert inst.set_overlap_post(True)
            else:
                assert inst.set_cu_split("post=0:2,sum=2:8,main=10:22")
            assert inst.reset(w, h, opt)
            outs = []
            for _ in range(2):
                assert inst.reset(w, h, opt)
                outs.append(inst.match_confidence(left, right))
            for dd, cc in outs:
                assert_same(dd, ref_disp, f"{setup}: disparity")
                assert_same(cc, ref_conf, f"{setup}: confidence")
        finally:
            inst.close()
    # the default instance (SGM_MatchConfidence), frame 0
    g = S.SGM()
    g.shutdown()
    try:
        assert g.initialize(w, h, opt)
        got = g.match_confidence(left[0], right[0])
        assert got is not None
        assert_same(got[0], ref_disp[0], "SGM_MatchConfidence: disparity")
        assert_same(got[1], ref_conf[0], "SGM_MatchConfidence: confidence")
    finally:
        g.shutdown()


def test_fused_last_sweep_is_skipped(monkeypatch):
    monkeypatch.setenv("SGM_UPSUM", "1")
    wl, _, left, right = _kitti_frames()
    w, h, d, B = wl["w"], wl["h"], wl["d"], 8
    opt = default_option(d)
    inst = new_instance(batch=B)
    try:
        assert inst.reset(w, h, opt)
        plain = inst.match(left, right)
        assert inst.fused_sweep_rows() > 0
        assert inst.reset(w, h, opt)
        disp, conf = inst.match_confidence(left, right)
        assert inst.fused_sweep_rows() == 0
        assert_same(disp, plain, "SGM_UPSUM=1: confidence match vs fused-sweep plain match")
        assert inst.reset(w, h, opt)
        assert_same(inst.match(left, right), plain, "plain match after a confidence match")
        assert inst.fused_sweep_rows() > 0
    finally:
        inst.close()


def test_row_tile_mode_refuses():
    left = np.zeros((20, 48), np.uint8)
    inst = new_instance()
    try:
        assert inst.set_rows(0, 10) and inst.reset(48, 20, default_option(16))
        assert inst.match_confidence(left, left) is None
    finally:
        inst.close()


def test_sgm_main_confidence_pgm(tmp_path, oracle):
    from PIL import Image
    z = load_npz("cone_inputs.npz")
    exe = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
    Image.fromarray(z["left"]).save(str(tmp_path / "l.png"))
    Image.fromarray(z["right"]).save(str(tmp_path / "r.png"))
    raw, pgm = str(tmp_path / "d.f32"), str(tmp_path / "c.pgm")
    subprocess.check_call([exe, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(tmp_path / "d.png"), "--raw", raw,
                           "--confidence", pgm], stdout=subprocess.DEVNULL, timeout=120)
    with open(pgm, "rb") as f:
        data = f.read()
    header = b"P5\n450 375\n65535\n"
    assert data.startswith(header) and len(data) == len(header) + 2 * 450 * 375
    conf = np.frombuffer(data[len(header):], ">u2").reshape(375, 450)
    opt = default_option(64)
    want = R.confidence(oracle_aggr(oracle, z["left"], z["right"], opt))[3]
    assert_same(conf.astype(np.uint16), want, "sgm_main --confidence")
    assert_same(np.fromfile(raw, np.float32).reshape(375, 450), load_npz("cone_final.npz")["final"], "sgm_main --confidence: disparity")
