"""Rectification on the device (extension; include/sgm_mi355x.h, SGM_SetRectify) against its numpy restatement
tests/rectify_ref.py -- needs an MI355X.  Tolerance 0 everywhere: the remap is integer arithmetic, and a match of a raw pair with
rectification on is, at every stage, the oracle's pipeline on the restatement's remap of that pair."""
import numpy as np
import pytest

import census_sym_ref as CS
import confidence_ref as CR
import fill_holes_ref as FH
import rectify_ref as RR
import refine_ref as RF
from oracle.pyoracle import STAGE_NAMES, Oracle, default_option
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def identity(w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x, y


def noise(w, h, seed, frames=None):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if frames is None else (frames, h, w), dtype=np.uint8)


def kernel_maps(w, h):
    """name -> (map_x, map_y): what the kernel has to get right, one at a time"""
    x, y = identity(w, h)
    K = RR.camera(w, h)
    rng = np.random.default_rng(w * 1000 + h)
    sx, sy = x + np.float32(0.3), y + np.float32(0.7)
    for v in (np.nan, np.inf, -np.inf, 1e9, -1e9):
        sx[rng.integers(0, h, 6), rng.integers(0, w, 6)] = v
        sy[rng.integers(0, h, 6), rng.integers(0, w, 6)] = v
    sx[h - 1, w - 1], sy[0, 0] = np.nan, np.inf                   # the very last and the very first entry
    return {
        "identity": (x, y),
        "shift": (x + 3, y - 2),
        "weights": (x + (x % 32) / 32, y + (y % 32) / 32),        # all 1024 weight pairs once H >= 32, W >= 32
        "rotation30": RR.maps(K, np.zeros(5), RR.rotation_z(30.0), K, w, h),
        "radial": RR.model_maps(RR.RADIAL, w, h),
        "outside": (x + 1000, y - 1000),
        "sprinkled": (sx, sy),
    }


SHAPES = [(70, 33), (130, 40), (20, 31), (24, 70), (33, 33)]     # W x H: W % 4 != 0, N % 4 in {0, 1, 2}, W < H


@pytest.mark.parametrize("w,h", SHAPES)
def test_kernel_equals_the_restatement(w, h):
    """sgm_rectify on device images with a canary behind each output, and stages 19 / 20 of a match, for every map and both kinds
    of image; the left and the right view get different maps (the right one's are the left one's mirrored)."""
    import torch
    import soc_project_stereo_matching_amd as S
    opt = S.default_option(8)
    n = w * h
    images = {"noise": (noise(w, h, 11), noise(w, h, 12)), "all255": (np.full((h, w), 255, np.uint8),) * 2}
    maps = kernel_maps(w, h)
    if w >= 32 and h >= 32:
        xq, yq = RR.quantise(*maps["weights"])
        assert len(set(zip((xq & 31).ravel().tolist(), (yq & 31).ravel().tolist()))) == 1024
    inst = S.SGMInstance(0)
    try:
        for name, (mx, my) in maps.items():
            rx, ry = np.ascontiguousarray(mx[:, ::-1]), np.ascontiguousarray(my[::-1, :])
            assert inst.set_rectify(mx, my, rx, ry), name
            assert inst.reset(w, h, opt), name
            for kind, (left, right) in images.items():
                want_l, want_r = RR.remap(left, mx, my), RR.remap(right, rx, ry)
                if name == "outside":
                    assert not want_l.any() and not want_r.any()
                d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
                out = torch.full((2, n + 8), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert inst.rectify(d_l.data_ptr(), d_r.data_ptr(), out[0].data_ptr(), out[1].data_ptr()) and inst.synchronize()
                got = out.cpu().numpy()
                assert np.all(got[:, n:] == 0xA5), f"{name} {kind}: wrote past the image"
                assert_same(got[0, :n].reshape(h, w), want_l, f"{w}x{h} {name} {kind}: left")
                assert_same(got[1, :n].reshape(h, w), want_r, f"{w}x{h} {name} {kind}: right")
                assert_same(d_l.cpu().numpy(), left, "the source is only read")
                if kind == "noise":
                    assert inst.match(left, right) is not None
                    got_l, got_r = inst.read_rectified()
                    assert_same(got_l, want_l, f"{w}x{h} {name}: stage 19")
                    assert_same(got_r, want_r, f"{w}x{h} {name}: stage 20")
    finally:
        inst.close()


@pytest.mark.parametrize("w,h", [(70, 33), (33, 33), (130, 40)])
def test_batch_of_three_under_one_set_of_maps(w, h):
    """Three different frames: frame f of the output is the remap of frame f (a wrong frame stride would mix them); W * H % 4 is
    2, 1 and 0, so the frames' offsets take the kernel through its dword, word and byte stores."""
    import torch
    import soc_project_stereo_matching_amd as S
    left, right = noise(w, h, 21, frames=3), noise(w, h, 22, frames=3)
    lx, ly = RR.model_maps(RR.ROTATED, w, h)
    rx, ry = RR.model_maps(RR.RADIAL, w, h)
    inst = S.SGMInstance(0, batch=3)
    try:
        assert inst.set_rectify(lx, ly, rx, ry) and inst.reset(w, h, S.default_option(8))
        d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        out = torch.full((2, 3 * w * h + 8), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert inst.rectify(d_l.data_ptr(), d_r.data_ptr(), out[0].data_ptr(), out[1].data_ptr()) and inst.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[:, 3 * w * h:] == 0x5A)
        assert_same(got[0, :3 * w * h].reshape(3, h, w), RR.remap(left, lx, ly), "left frames")
        assert_same(got[1, :3 * w * h].reshape(3, h, w), RR.remap(right, rx, ry), "right frames")
        assert inst.match(left, right) is not None
        for f in range(3):
            inst.select_frame(f)
            got_l, got_r = inst.read_rectified()
            assert_same(got_l, RR.remap(left[f], lx, ly), f"stage 19 of frame {f}")
            assert_same(got_r, RR.remap(right[f], rx, ry), f"stage 20 of frame {f}")
    finally:
        inst.close()


@pytest.mark.parametrize("name", ["t70x33_d16", "t40x24_d16_dmin3"])
def test_identity_maps_change_nothing(oracle, golden_cases, name):
    import soc_project_stereo_matching_amd as S
    from conftest import case_inputs, option_from_dict
    case = golden_cases[name]
    left, right = case_inputs(case, oracle)
    opt = option_from_dict(case["option"])
    w, h = case["w"], case["h"]
    want = oracle.run(left, right, opt)
    inst = S.SGMInstance(0)
    try:
        inst.keep_stages(True)
        x, y = identity(w, h)
        assert inst.set_rectify(x, y, x, y) and inst.reset(w, h, opt)
        out = inst.match(left, right)
        st = inst.read_stages()
        for n in STAGE_NAMES:
            assert_same(st[n], want[n], f"{name}: stage {n} under identity maps")
        assert_same(out, want["final"], f"{name}: result under identity maps")
        got_l, got_r = inst.read_rectified()
        assert_same(got_l, left, "stage 19")
        assert_same(got_r, right, "stage 20")
    finally:
        inst.close()


# ---- non-trivial maps: a small rotation plus radial, the two cameras rolled against each other ---------------------------

class Rig:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.lx, self.ly = RR.model_maps(RR.SMALL, w, h)
        self.rx, self.ry = RR.model_maps(RR.SMALL, w, h, sign=-1.0)

    def on(self, inst):
        return inst.set_rectify(self.lx, self.ly, self.rx, self.ry)

    def rectified(self, left, right):
        return RR.remap(left, self.lx, self.ly), RR.remap(right, self.rx, self.ry)


def raw_pair(oracle, w, h, d, seed):
    return oracle.synth_pair(w, h, d, seed)


@pytest.mark.parametrize("w,h,dmin,dmax", [(70, 33, 0, 16), (64, 20, 0, 40), (20, 31, 0, 8)])
def test_plain_match_equals_the_oracle_on_the_rectified_pair(oracle, w, h, dmin, dmax):
    import soc_project_stereo_matching_amd as S
    left, right = raw_pair(oracle, w, h, dmax - dmin, 0x4EC7 + w)
    opt = default_option(dmax, dmin, min_speckle_area=10)
    rig = Rig(w, h)
    rl, rr = rig.rectified(left, right)
    assert not np.array_equal(rl, left)
    want = oracle.run(rl, rr, opt)
    inst = S.SGMInstance(0)
    try:
        inst.keep_stages(True)
        assert rig.on(inst) and inst.reset(w, h, opt)
        out = inst.match(left, right)
        st = inst.read_stages()
        for n in STAGE_NAMES:
            assert_same(st[n], want[n], f"{w}x{h}: stage {n}")
        assert_same(out, want["final"], f"{w}x{h}: result")
    finally:
        inst.close()


def test_symmetric_census_7x7(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    left, right = raw_pair(oracle, w, h, d, 0x4EC8)
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    want = CS.pipeline(oracle, *rig.rectified(left, right), opt, 7, 7)
    inst = S.SGMInstance(0)
    try:
        inst.keep_stages(True)
        assert inst.set_census_window(7, 7) and inst.set_census_kind(S.sgm.CENSUS_SYMMETRIC)
        assert rig.on(inst) and inst.reset(w, h, opt)
        out = inst.match(left, right)
        st = inst.read_stages()
        for n in STAGE_NAMES:
            assert_same(st[n], want[n], f"symmetric 7x7: stage {n}")
        assert_same(out, want["final"], "symmetric 7x7: result")
    finally:
        inst.close()


def test_batch_of_three_matches(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    pairs = [raw_pair(oracle, w, h, d, 0x4ED0 + j) for j in range(3)]
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    inst = S.SGMInstance(0, batch=3)
    try:
        assert rig.on(inst) and inst.reset(w, h, opt)
        out = inst.match(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
        for j, (l, r) in enumerate(pairs):
            assert_same(out[j], oracle.run(*rig.rectified(l, r), opt)["final"], f"frame {j}")
    finally:
        inst.close()


def test_right_reference_view_and_match_both(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    left, right = raw_pair(oracle, w, h, d, 0x4ED8)
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    rl, rr = rig.rectified(left, right)
    want_l = oracle.run(rl, rr, opt)
    oracle.set_reference_view(True)
    try:
        want_r = oracle.run(rl, rr, opt)
    finally:
        oracle.set_reference_view(False)
    inst = S.SGMInstance(0)
    try:
        assert rig.on(inst) and inst.reset(w, h, opt)
        both = inst.match_both(left, right)
        assert both is not None
        assert_same(both[0], want_l["final"], "match_both: left map")
        assert_same(both[1], want_r["final"], "match_both: right map")
        inst.set_reference_view(True)
        inst.keep_stages(True)
        assert inst.reset(w, h, opt)
        out = inst.match(left, right)
        assert_same(inst.read_stage("disp_r"), want_r["disp_r"], "right view: WTA")
        assert_same(out, want_r["final"], "right view: result")
    finally:
        inst.close()


def test_confidence_fill_and_refinement(oracle):
    """The confidence of the rectified pair's costs; hole filling on it; the refinement, whose guide must be the RECTIFIED
    reference image (refine_ref fed the raw image gives another map)."""
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    left, right = raw_pair(oracle, w, h, d, 0x4EE0)
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    rl, rr = rig.rectified(left, right)
    st = oracle.run(rl, rr, opt)
    conf = CR.confidence(st["aggr"], opt.min_disparity, False)[3]
    inst = S.SGMInstance(0)
    try:
        assert rig.on(inst) and inst.reset(w, h, opt)
        got = inst.match_confidence(left, right)
        assert got is not None
        assert_same(got[0], st["final"], "match_confidence: map")
        assert_same(got[1], conf, "match_confidence: confidence")
        assert inst.set_fill_holes(True) and inst.reset(w, h, opt)
        assert_same(inst.match(left, right), FH.expected(st, opt, oracle)[2], "hole filling")
        assert inst.set_fill_holes(False)
        assert inst.set_refine(True) and inst.reset(w, h, opt)
        tabs = RF.tables(S.REFINE_LAMBDA, S.REFINE_SIGMA, S.REFINE_ITERS, S.load_library())
        want = RF.refine(st["final"], conf, rl, tabs)
        assert not np.array_equal(want.view(np.uint32), RF.refine(st["final"], conf, left, tabs).view(np.uint32))
        assert_same(inst.match(left, right), want, "refinement guided by the rectified image")
    finally:
        inst.close()


def test_two_matches_without_reset(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    pairs = [raw_pair(oracle, w, h, d, 0x4EE8 + j) for j in range(2)]
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    orc = Oracle()
    inst = S.SGMInstance(0)
    try:
        assert orc.reset(w, h, opt) and rig.on(inst) and inst.reset(w, h, opt)
        for k, (l, r) in enumerate(pairs):
            assert_same(inst.match(l, r), orc.match(*rig.rectified(l, r)), f"match {k} without Reset")
    finally:
        inst.close()


def test_match_planes_is_grey_then_remap(oracle):
    import soc_project_stereo_matching_amd as S
    from oracle.platform_oracle import board_gray, disparity_to_depth
    from test_gpu_parity import _colour_planes
    w, h, d = 70, 33, 16
    fx, baseline, doffs = 1733.74, 536.62, 0.0
    planes = _colour_planes(oracle, w, h, d, 0x4EF0, np.random.default_rng(5))
    rig = Rig(w, h)
    gl, gr = board_gray(planes[0], planes[1], planes[2]), board_gray(planes[3], planes[4], planes[5])
    disp = oracle.run(*rig.rectified(gl, gr), default_option(d))["final"]
    want = disparity_to_depth(disp, fx, baseline, doffs)
    inst = S.SGMInstance(0)
    try:
        assert rig.on(inst) and inst.reset(w, h, S.default_option(d))
        depth = np.empty((h, w), np.float32)
        assert inst.match_planes(np.ascontiguousarray(planes), fx, baseline, doffs, depth)
        assert_same(inst.read_stage("final"), disp, "disparity behind the depth map")
        assert np.array_equal(np.isnan(depth), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(depth[ok].view(np.uint32), want[ok].view(np.uint32))
    finally:
        inst.close()


def test_match_device_and_two_pairs_in_flight(oracle):
    """Device-resident raw images are only read; with the post pass on its own stream two different pairs are queued back to back
    without a wait between them: the remap of the second must not overtake anything that still reads the first's rectified
    images."""
    import torch
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    pairs = [raw_pair(oracle, w, h, d, 0x4EF8 + j) for j in range(2)]
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    inst = S.SGMInstance(0)
    try:
        assert inst.set_overlap_post(True) and rig.on(inst)
        ins = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in pairs]
        outs = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in pairs]
        torch.cuda.synchronize()
        for k in range(2):
            assert inst.reset(w, h, opt)
            assert inst.match_device(ins[k][0].data_ptr(), ins[k][1].data_ptr(), outs[k].data_ptr())
        assert inst.synchronize()
        for k, (l, r) in enumerate(pairs):
            assert_same(outs[k].cpu().numpy(), oracle.run(*rig.rectified(l, r), opt)["final"], f"pair {k} in flight")
            assert_same(ins[k][0].cpu().numpy(), l, "the caller's raw left image")
            assert_same(ins[k][1].cpu().numpy(), r, "the caller's raw right image")
    finally:
        inst.close()


def test_fused_sweep_reads_the_rectified_copy(oracle, monkeypatch):
    """The opt-in fused last sweep (set up as tests/test_gpu_upsum.py does) keeps a copy of the left image for its own kernel and for
    S re-created afterwards: the rectified one."""
    import soc_project_stereo_matching_amd as S
    monkeypatch.setenv("SGM_UPSUM", "1")
    w, h, d = 300, 40, 128
    opt = default_option(d, min_speckle_area=10)
    pairs = [raw_pair(oracle, w, h, d, 0x4F00 + j) for j in range(2)]
    rig = Rig(w, h)
    inst = S.SGMInstance(0, batch=2)
    try:
        assert rig.on(inst) and inst.reset(w, h, opt)
        out = inst.match(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
        assert out is not None and inst.fused_sweep_rows() == 3
        for j, (l, r) in enumerate(pairs):
            want = oracle.run(*rig.rectified(l, r), opt)
            inst.select_frame(j)
            assert_same(out[j], want["final"], f"fused sweep, frame {j}: final")
            assert_same(inst.read_stage("aggr"), want["aggr"], f"fused sweep, frame {j}: S after the fact")
    finally:
        inst.close()


def test_changing_the_maps(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    left, right = raw_pair(oracle, w, h, d, 0x4F08)
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    x, y = identity(w, h)
    inst = S.SGMInstance(0)
    try:
        assert rig.on(inst) and inst.reset(w, h, opt)
        assert_same(inst.match(left, right), oracle.run(*rig.rectified(left, right), opt)["final"], "first maps")
        # new maps: not before a reset, then they rule
        assert inst.set_rectify(x + 2, y + 1, x - 1, y)
        assert inst.reset(w, h, opt)
        want = oracle.run(RR.remap(left, x + 2, y + 1), RR.remap(right, x - 1, y), opt)["final"]
        assert_same(inst.match(left, right), want, "second maps")
        # maps of the wrong shape: reset refuses, and matching needs a good one again
        x2, y2 = identity(w + 1, h)
        assert inst.set_rectify(x2, y2, x2, y2)
        assert not inst.reset(w, h, opt)
        # off: the plain match, no stages 19 / 20
        assert inst.set_rectify(None) and inst.reset(w, h, opt)
        assert_same(inst.match(left, right), oracle.run(left, right, opt)["final"], "rectification off")
        with pytest.raises(RuntimeError):
            inst.read_rectified()
        assert not inst.rectify(0, 0, 0, 0)
    finally:
        inst.close()


def test_default_instance(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    left, right = raw_pair(oracle, w, h, d, 0x4F10)
    opt = default_option(d, min_speckle_area=10)
    rig = Rig(w, h)
    g = S.SGM()
    g.shutdown()
    try:
        assert g.set_rectify(rig.lx, rig.ly, rig.rx, rig.ry)
        want = oracle.run(*rig.rectified(left, right), opt)["final"]
        assert g.reset(w, h, opt)
        assert_same(g.match(left, right), want, "SGM_Match with SGM_SetRectify")
        g.shutdown()                                              # remembered across a shutdown
        assert g.reset(w, h, opt)
        assert_same(g.match(left, right), want, "after SGM_Shutdown")
        assert g.set_rectify(None) and g.reset(w, h, opt)
        assert_same(g.match(left, right), oracle.run(left, right, opt)["final"], "off again")
    finally:
        g.set_rectify(None)
        g.shutdown()


def _calib_file(path, w, h):
    """CALIB.txt of the drivers: K dist R Knew of the left camera, then of the right one (the SMALL model, rolled both ways)"""
    with open(path, "w") as f:
        for sign in (1.0, -1.0):
            for m in RR.model(RR.SMALL, w, h, sign):
                f.write(" ".join(repr(float(v)) for v in np.asarray(m, np.float64).ravel()) + "\n")


def test_drivers_rectify_flag(tmp_path, oracle):
    """sgm_main --rectify CALIB.txt --rectified-out: the map and the two rectified images of the oracle on the restatement's remap;
    sgm_stream --rectify runs and reports a map other than without."""
    import json
    import os
    import subprocess
    from PIL import Image
    from conftest import ROOT
    w, h, d = 203, 77, 64
    left, right = raw_pair(oracle, w, h, d, 0x4F18)
    Image.fromarray(left).save(str(tmp_path / "l.png"))
    Image.fromarray(right).save(str(tmp_path / "r.png"))
    calib = str(tmp_path / "calib.txt")
    _calib_file(calib, w, h)
    rig = Rig(w, h)
    rl, rr = rig.rectified(left, right)
    exe = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
    raw = str(tmp_path / "d.f32")
    subprocess.check_call([exe, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(tmp_path / "d.png"), "--raw", raw, "--max-disparity",
                           str(d), "--rectify", calib, "--rectified-out", str(tmp_path / "rl.pgm"), str(tmp_path / "rr.pgm")],
                          stdout=subprocess.DEVNULL, timeout=120)
    assert_same(np.asarray(Image.open(str(tmp_path / "rl.pgm"))), rl, "sgm_main: rectified left")
    assert_same(np.asarray(Image.open(str(tmp_path / "rr.pgm"))), rr, "sgm_main: rectified right")
    assert_same(np.fromfile(raw, np.float32).reshape(h, w), oracle.run(rl, rr, default_option(d, min_speckle_area=50))["final"], "sgm_main --rectify")
    with open(str(tmp_path / "short.txt"), "w") as f:
        f.write("1 2 3\n")
    bad = subprocess.run([exe, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(tmp_path / "d.png"), "--rectify", str(tmp_path / "short.txt")],
                         capture_output=True, timeout=60)
    assert bad.returncode != 0
    stream = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_stream")
    common = [stream, "--width", str(w), "--height", str(h), "--disparities", str(d), "--batch", "2", "--instances", "2", "--frames", "4",
              "--seconds", "0.2"]
    lines = [json.loads(subprocess.run(common + extra, capture_output=True, text=True, timeout=120, check=True).stdout.strip().splitlines()[-1])
             for extra in ([], ["--rectify", calib])]
    assert lines[0]["hash_frame0"] != lines[1]["hash_frame0"]
