"""Refinement on the device (include/sgm_mi355x.h, SGM_SetRefine; csrc/sgm_refine.hip) -- needs an MI355X.

Parity unpinned by the reference (it has no such stage): the expected map is the numpy restatement tests/refine_ref.py, with the
library's weight tables, applied to the disparity map and the confidence of a second instance with the refinement off running the
same sequence through sgm_match_confidence* (itself pinned against the oracle by tests/test_gpu_confidence.py), guided by the
reference view's image.  Tolerance: 0 -- bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import refine_ref as R
from conftest import ROOT, load_npz
from oracle.pyoracle import default_option

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={np.asarray(got)[first]} "
                             f"want={np.asarray(want)[first]}")


def defaults():
    import soc_project_stereo_matching_amd as S
    return (S.REFINE_LAMBDA, S.REFINE_SIGMA, S.REFINE_ITERS)


def expected(disp, conf, guide, params, keep=False):
    import soc_project_stereo_matching_amd as S
    lam, sigma, T = params
    return R.refine(disp, conf, guide, R.tables(lam, sigma, T, S.load_library()), keep)


class Pair:
    """A refining instance and a plain one with the same options, view and batch."""

    def __init__(self, params=None, keep=False, batch=1, right_view=False, honor=False, window=(5, 5)):
        import soc_project_stereo_matching_amd as S
        self.params = params or defaults()
        self.keep = keep
        self.right_view = right_view
        self.ref = S.SGMInstance(0, batch=batch)
        self.plain = S.SGMInstance(0, batch=batch)
        for i in (self.ref, self.plain):
            i.set_reference_view(right_view)
            i.set_honor_num_paths(honor)
            assert i.set_census_window(*window)
        assert self.ref.set_refine(True, *self.params, keep_invalid=keep)

    def reset(self, w, h, opt):
        assert self.ref.reset(w, h, opt) and self.plain.reset(w, h, opt)

    def want(self, left, right):
        """the plain instance's map and confidence of this match, refined in numpy"""
        got = self.plain.match_confidence(left, right)
        assert got is not None
        return expected(got[0], got[1], right if self.right_view else left, self.params, self.keep), got[0]

    def check(self, left, right, opt, what):
        h, w = left.shape[-2:]
        self.reset(w, h, opt)
        got = self.ref.match(left, right)
        assert got is not None, what
        want, plain = self.want(left, right)
        assert_same(got, want, what)
        return got, plain

    def close(self):
        self.ref.close()
        self.plain.close()


@pytest.mark.parametrize("right_view", [False, True], ids=["left", "right"])
def test_cone_reference_options(right_view):
    z = load_npz("cone_inputs.npz")
    p = Pair(right_view=right_view)
    try:
        got, plain = p.check(z["left"], z["right"], default_option(64), f"cone right={right_view}")
        assert np.isinf(plain).any() and np.isfinite(got).mean() > np.isfinite(plain).mean()
    finally:
        p.close()


VARIANTS = {
    "dmin5": dict(w=150, h=60, d=32, dmin=5),
    "no_unique": dict(w=150, h=60, d=32, opt=dict(is_check_unique=False)),
    "no_lr": dict(w=150, h=60, d=32, opt=dict(is_check_lr=False)),
    "paths4": dict(w=150, h=60, d=32, honor=True, opt=dict(num_paths=4)),
    "census7x7": dict(w=120, h=48, d=32, window=(7, 7)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_option_variants(oracle, name):
    v = VARIANTS[name]
    dmin = v.get("dmin", 0)
    left, right = oracle.synth_pair(v["w"], v["h"], v["d"] + dmin, 0x5EF0 + len(name))
    opt = default_option(v["d"] + dmin, dmin, **v.get("opt", {}))
    for right_view in (False, True):
        p = Pair(right_view=right_view, honor=v.get("honor", False), window=v.get("window", (5, 5)))
        try:
            p.check(left, right, opt, f"{name} right={right_view}")
        finally:
            p.close()


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_iterations_keep_invalid_and_underflow(oracle, T):
    left, right = oracle.synth_pair(203, 77, 64, 0x7E + T)
    opt = default_option(64)
    for params in ((24.0, 6.0, T), (200.0, 0.4, T)):               # sigma 0.4: exp(-k / 0.4) underflows from k = 42 on
        for keep in (False, True):
            p = Pair(params=params, keep=keep)
            try:
                got, plain = p.check(left, right, opt, f"T={T} params={params} keep={keep}")
                if keep:                                           # (a valid pixel can still end without weight: V = 0)
                    assert np.isinf(got[np.isinf(plain)]).all()
            finally:
                p.close()


def test_q14_match_without_reset():
    z = load_npz("cone_inputs.npz")
    opt = default_option(64)
    p = Pair()
    try:
        p.reset(450, 375, opt)
        assert p.ref.match(z["left"], z["right"]) is not None
        got = p.ref.match(z["left"], z["right"])
        assert p.plain.match_confidence(z["left"], z["right"]) is not None
        want, _ = p.want(z["left"], z["right"])
        assert_same(got, want, "Q14: second match without reset")
    finally:
        p.close()


def _kitti_frames(n=8, first=0):
    with open(os.path.join(ROOT, "tests", "golden", "bench_frames.json")) as f:
        wl = json.load(f)["workloads"]["kitti_1242x375_d128_p8"]
    import soc_project_stereo_matching_amd as S
    pairs = [S.synth_pair(wl["w"], wl["h"], wl["d"], wl["first_seed"] + first + k) for k in range(n)]
    return wl, np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])


def test_kitti_batch_of_8():
    wl, left, right = _kitti_frames()
    p = Pair(batch=8)
    try:
        got, plain = p.check(left, right, default_option(wl["d"]), "kitti batch of 8")
        assert np.isfinite(got).all() or np.isfinite(got).mean() > np.isfinite(plain).mean()
    finally:
        p.close()


def test_overlapped_post_sequence_of_distinct_frames():
    """Distinct frames back to back with overlapped post passes: through sgm_match_async, and through device pointers whose image
    buffers the caller rewrites on the instance's stream right after each match is queued -- while that match's refinement may
    still be running on the post stream.  Each result must be exact (the refinement reads a private copy of the guide)."""
    import torch
    wl, left, right = _kitti_frames(n=8)
    w, h, d, B, N = wl["w"], wl["h"], wl["d"], 2, 4
    left, right = left.reshape(N, B, h, w), right.reshape(N, B, h, w)
    opt = default_option(d)
    p = Pair(batch=B)
    try:
        assert p.ref.set_overlap_post(True)
        p.reset(w, h, opt)
        wants = []
        for i in range(N):
            assert p.plain.reset(w, h, opt)
            wants.append(p.want(left[i], right[i])[0])
        # host pointers, pipelined
        outs = [np.empty((B, h, w), np.float32) for _ in range(N)]
        for i in range(N):
            assert p.ref.reset(w, h, opt) and p.ref.match_async(left[i], right[i], outs[i])
        assert p.ref.match_wait()
        for i in range(N):
            assert_same(outs[i], wants[i], f"match_async sequence, match {i}")
        # device pointers: one pair of image buffers, rewritten on the instance's stream between the matches
        src_l, src_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        img_l, img_r = torch.empty_like(src_l[0]), torch.empty_like(src_r[0])
        touts = [torch.empty((B, h, w), dtype=torch.float32, device="cuda") for _ in range(N)]
        torch.cuda.synchronize()
        st = torch.cuda.ExternalStream(p.ref.stream)
        for i in range(N):
            with torch.cuda.stream(st):
                img_l.copy_(src_l[i])
                img_r.copy_(src_r[i])
            assert p.ref.reset(w, h, opt)
            assert p.ref.match_device(img_l.data_ptr(), img_r.data_ptr(), touts[i].data_ptr())
        with torch.cuda.stream(st):
            img_l.zero_()
            img_r.zero_()
        assert p.ref.synchronize()
        for i in range(N):
            assert_same(touts[i].cpu().numpy(), wants[i], f"device sequence, match {i}")
    finally:
        p.close()


def test_entry_points():
    """sgm_match_confidence* (refined map + the confidence), device pointers, SGM_Match / sgm_compute of the default instance and
    the depth of sgm_match_planes."""
    import torch
    import soc_project_stereo_matching_amd as S
    from oracle.platform_oracle import board_gray
    wl, left, right = _kitti_frames(n=2)
    w, h, d, B = wl["w"], wl["h"], wl["d"], 2
    opt = default_option(d)
    p = Pair(batch=B)
    try:
        p.reset(w, h, opt)
        want, _ = p.want(left, right)
        assert p.plain.reset(w, h, opt)
        conf_plain = p.plain.match_confidence(left, right)[1]
        assert p.ref.reset(w, h, opt)
        disp, conf = p.ref.match_confidence(left, right)
        assert_same(disp, want, "sgm_match_confidence: disparity")
        assert np.array_equal(conf, conf_plain)
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        td = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        tc = torch.zeros((B, h, w), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert p.ref.reset(w, h, opt) and p.ref.match_device(tl.data_ptr(), tr.data_ptr(), td.data_ptr()) and p.ref.synchronize()
        assert_same(td.cpu().numpy(), want, "sgm_match_device")
        assert p.ref.reset(w, h, opt)
        assert p.ref.match_confidence_device(tl.data_ptr(), tr.data_ptr(), td.data_ptr(), tc.data_ptr()) and p.ref.synchronize()
        assert_same(td.cpu().numpy(), want, "sgm_match_confidence_device: disparity")
        assert np.array_equal(tc.cpu().numpy().view(np.uint16), conf_plain)
    finally:
        p.close()
    # the default instance
    g = S.SGM()
    g.shutdown()
    try:
        assert S.set_refine(True)
        assert_same(g.compute(left[0], right[0], opt), want[0], "sgm_compute with SGM_SetRefine")
        assert g.reset(w, h, opt)
        assert_same(g.match(left[0], right[0]), want[0], "SGM_Match with SGM_SetRefine")
        assert_same(g.match_confidence(left[0], right[0])[0], want[0], "SGM_MatchConfidence with SGM_SetRefine")
    finally:
        S.set_refine(False)
        g.shutdown()
    # sgm_match_planes: the depth of the refined map
    wp, hp, dp = 322, 97, 48
    fx, baseline, doffs = 1733.74, 536.62, 0.0
    rng = np.random.default_rng(3)
    l0, r0 = S.synth_pair(wp, hp, dp, 0x9A12)
    planes = np.stack([l0, np.clip(l0.astype(int) + rng.integers(-2, 3, l0.shape), 0, 255).astype(np.uint8), l0, r0, r0, r0])
    gl, gr = board_gray(planes[0], planes[1], planes[2]), board_gray(planes[3], planes[4], planes[5])
    p = Pair()
    try:
        p.reset(wp, hp, default_option(dp))
        depth = np.empty((hp, wp), np.float32)
        assert p.ref.match_planes(planes, fx, baseline, doffs, depth)
        want_p, _ = p.want(gl, gr)
        assert_same(p.ref.read_stage("final"), want_p, "sgm_match_planes: the disparity behind the depth")
        t_disp = torch.from_numpy(want_p).cuda()
        t_depth = torch.empty((hp, wp), dtype=torch.float32, device="cuda")
        assert p.ref.disparity_to_depth(t_disp.data_ptr(), want_p.size, fx, baseline, doffs, t_depth.data_ptr())
        assert p.ref.synchronize()
        assert_same(depth, t_depth.cpu().numpy(), "sgm_match_planes: depth of the refined map")
    finally:
        p.close()


def test_refine_disparity_on_crafted_maps():
    import torch
    import soc_project_stereo_matching_amd as S
    rng = np.random.default_rng(9)
    w, h, B = 77, 45, 3
    inst = S.SGMInstance(0, batch=B)
    try:
        assert inst.reset(w, h, default_option(16))                # refinement off for matches: the call works regardless
        disp = (rng.random((B, h, w)) * 60).astype(np.float32)
        disp[rng.random((B, h, w)) < 0.5] = INF
        disp[1] = INF                                             # a frame with nothing valid
        conf = rng.integers(0, 65536, (B, h, w)).astype(np.uint16)
        conf[2, :, :20] = 0
        guide = rng.integers(0, 256, (B, h, w)).astype(np.uint8)
        guide[0, :, 40:] //= 4
        for params, keep in (((16.0, 1.5, 1), False), ((64.0, 8.0, 3), True), ((500.0, 0.3, 8), False)):
            assert inst.set_refine(True, *params, keep_invalid=keep)
            td = torch.from_numpy(disp.copy()).cuda()
            tc = torch.from_numpy(conf.view(np.int16)).cuda()
            tg = torch.from_numpy(guide).cuda()
            assert inst.refine_disparity(td, tc, tg) and inst.synchronize()
            got = td.cpu().numpy()
            assert_same(got, expected(disp, conf, guide, params, keep), f"crafted maps {params} keep={keep}")
            assert np.isinf(got[1]).all()
        # a KITTI-sized map that is +INF everywhere stays +INF
        k = S.SGMInstance(0)
        try:
            assert k.reset(1242, 375, default_option(128)) and k.set_refine(True)
            td = torch.full((375, 1242), float("inf"), dtype=torch.float32, device="cuda")
            tc = torch.full((375, 1242), -1, dtype=torch.int16, device="cuda")      # 65535
            tg = torch.zeros((375, 1242), dtype=torch.uint8, device="cuda")
            assert k.refine_disparity(td, tc, tg) and k.synchronize()
            assert bool(torch.isinf(td).all())
        finally:
            k.close()
    finally:
        inst.close()


def test_refinement_off_again_gives_the_plain_map(oracle):
    left, right = oracle.synth_pair(203, 77, 64, 0xAB)
    opt = default_option(64)
    p = Pair()
    try:
        refined, plain = p.check(left, right, opt, "refinement on")
        assert p.ref.set_refine(False) and p.ref.reset(203, 77, opt)
        got = p.ref.match(left, right)
        assert_same(got, oracle.run(left, right, opt)["final"], "refinement off again vs the oracle")
        assert_same(got, plain, "refinement off again vs the plain instance")
        assert not np.array_equal(np.isinf(refined), np.isinf(got))
    finally:
        p.close()


def test_sgm_main_refine_flag(tmp_path, oracle):
    from PIL import Image
    exe = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
    w, h, d = 203, 77, 64
    left, right = oracle.synth_pair(w, h, d, 0xC12)
    Image.fromarray(left).save(str(tmp_path / "l.png"))
    Image.fromarray(right).save(str(tmp_path / "r.png"))
    for flag, params in (("--refine", defaults()), ("--refine=40,3,2", (40.0, 3.0, 2))):
        raw = str(tmp_path / "d.f32")
        subprocess.check_call([exe, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(tmp_path / "d.png"), "--raw", raw,
                               "--max-disparity", str(d), flag], stdout=subprocess.DEVNULL, timeout=120)
        p = Pair(params=params)
        try:
            p.reset(w, h, default_option(d))
            want, _ = p.want(left, right)
        finally:
            p.close()
        assert_same(np.fromfile(raw, np.float32).reshape(h, w), want, f"sgm_main {flag}")
    r = subprocess.run([exe, str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(tmp_path / "d.png"), "--refine=1,2"],
                       capture_output=True, timeout=60)
    assert r.returncode == 2
