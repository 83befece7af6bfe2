"""The centre-symmetric census (SGM_SetCensusKind, include/sgm_mi355x.h) on an MI355X, through the C-ABI: every stage of a
match bit-identical to tests/census_sym_ref.py's pipeline() -- the numpy census feeding the oracle's own stage functions --
for every window class and block layout of sgm_census_sym_k, for everything the 5x5 fast path composes with, and the proof
that it IS the fast path (u32 words, no cost volume).  Parity unpinned by the reference; tolerance 0."""
import numpy as np
import pytest

import census_sym_ref as CS
import confidence_ref as CR
from oracle.pyoracle import STAGE_NAMES, default_option
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SYM = 1
WINDOWS = [(5, 5), (7, 7), (9, 7), (3, 21), (21, 3), (63, 1), (1, 63)]
SHAPES = [(70, 33, 0, 16),        # two blocks across, three down, ragged
          (130, 40, 0, 16),       # three blocks across
          (20, 31, 0, 8),         # W < H
          (64, 20, 0, 40),        # padded disparity range
          (40, 24, 3, 19),        # dmin = 3, D = 16
          (24, 70, 0, 8)]         # tall enough for 1x63 and 3x21 to have an interior (five blocks down)


def sym_instance(cw, ch, batch=1, keep=True):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0, batch=batch)
    assert i.set_census_kind(SYM) and i.set_census_window(cw, ch)
    i.keep_stages(keep)
    return i


def check_stages(got, want, what):
    for n in STAGE_NAMES:
        if want[n] is not None:
            assert_same(got[n], want[n], f"{what}:{n}")


@pytest.fixture(scope="module")
def pairs(oracle):
    """one seeded pair per shape, shared (and left unchanged) by the window cases"""
    return {s: oracle.synth_pair(s[0], s[1], s[3] - s[2], 0xC5C0 + s[0] * 3 + s[1]) for s in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_d{s[2]}-{s[3]}")
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_every_stage_for_windows_and_shapes(oracle, pairs, window, shape):
    """Among them the frames with W <= cw or H <= ch (63x1 on 20x31 and 40x24, 1x63 on all but 24x70, 3x21 on 64x20): every
    word is zero and the pipeline still runs."""
    cw, ch = window
    w, h, dmin, dmax = shape
    left, right = pairs[shape]
    opt = default_option(dmax, dmin, min_speckle_area=9)
    want = CS.pipeline(oracle, left, right, opt, cw, ch)
    assert want["census_l"].any() == (w > cw and h > ch)
    i = sym_instance(cw, ch)
    try:
        assert i.reset(w, h, opt)
        out = i.match(left, right)
        assert out is not None
        check_stages(i.read_stages(), want, f"{window} {shape}")
        assert_same(out, want["final"], f"{window} {shape}:result")
    finally:
        i.close()


def test_batch_of_three_different_frames(oracle):
    w, h, d, B = 130, 40, 16, 3
    opt = default_option(d, min_speckle_area=9)
    frames = [oracle.synth_pair(w, h, d, 0xBA7C + k) for k in range(B)]
    i = sym_instance(9, 7, batch=B)
    try:
        assert i.reset(w, h, opt)
        out = i.match(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
        assert out is not None
        for k, (l, r) in enumerate(frames):
            want = CS.pipeline(oracle, l, r, opt, 9, 7)
            i.select_frame(k)
            check_stages(i.read_stages(), want, f"frame {k}")
            assert_same(out[k], want["final"], f"frame {k}:result")
    finally:
        i.close()


def test_honoured_four_path_mode(oracle):
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9, num_paths=4)
    left, right = oracle.synth_pair(w, h, d, 0x4A74)
    want = CS.pipeline(oracle, left, right, opt, 7, 7, honor_num_paths=True)
    assert not np.array_equal(want["aggr"], CS.pipeline(oracle, left, right, opt, 7, 7)["aggr"])
    i = sym_instance(7, 7)
    try:
        i.set_honor_num_paths(True)
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), want["final"], "four paths:result")
        check_stages(i.read_stages(), want, "four paths")
    finally:
        i.close()


def test_negative_p1_runs_the_generic_step(oracle):
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9, p1=-3, p2_init=40)
    left, right = oracle.synth_pair(w, h, d, 0x9E6)
    want = CS.pipeline(oracle, left, right, opt, 9, 7)
    i = sym_instance(9, 7)
    try:
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), want["final"], "P1 < 0:result")
        check_stages(i.read_stages(), want, "P1 < 0")
    finally:
        i.close()


def test_right_reference_view(oracle):
    w, h, d = 130, 40, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0x816)
    want = CS.pipeline(oracle, left, right, opt, 7, 7, right_view=True)
    i = sym_instance(7, 7)
    try:
        i.set_reference_view(True)
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), want["final"], "right view:result")
        check_stages(i.read_stages(), want, "right view")
    finally:
        i.close()


def test_match_both_equals_the_two_single_view_results(oracle):
    w, h, d = 130, 40, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0xB07)
    want_l = CS.pipeline(oracle, left, right, opt, 9, 7)["final"]
    want_r = CS.pipeline(oracle, left, right, opt, 9, 7, right_view=True)["final"]
    i = sym_instance(9, 7, keep=False)
    try:
        assert i.reset(w, h, opt)
        both = i.match_both(left, right)
        assert both is not None
        assert_same(both[0], want_l, "both: left")
        assert_same(both[1], want_r, "both: right")
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), both[0], "single left view")
        i.set_reference_view(True)
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), both[1], "single right view")
    finally:
        i.close()


def test_confidence_against_the_checkers_costs(oracle):
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0xC0F)
    want = CS.pipeline(oracle, left, right, opt, 7, 7)
    i = sym_instance(7, 7, keep=False)
    try:
        assert i.reset(w, h, opt)
        got = i.match_confidence(left, right)
        assert got is not None
        assert_same(got[0], want["final"], "confidence: map")
        assert_same(got[1], CR.confidence(want["aggr"], opt.min_disparity, False)[3], "confidence")
    finally:
        i.close()


def test_hole_filling_on_the_symmetric_maps(oracle):
    import fill_holes_ref as FH
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0xF111)
    want = CS.pipeline(oracle, left, right, opt, 7, 7)
    cls, filled, final = FH.expected(want, opt, oracle)
    i = sym_instance(7, 7)
    try:
        assert i.set_fill_holes(True) and i.reset(w, h, opt)
        got = i.match(left, right)
        assert_same(i.read_stage("after_speckle"), want["after_speckle"], "filling: stage 7")
        assert_same(i.read_fill_classes(), cls, "filling: classes")
        assert_same(i.read_filled(), filled, "filling: stage 9")
        assert_same(got, final, "filling: final")
    finally:
        i.close()


def test_refinement_of_the_symmetric_map(oracle):
    import refine_ref as R
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0x4EF1)
    want = CS.pipeline(oracle, left, right, opt, 7, 7)
    conf = CR.confidence(want["aggr"], opt.min_disparity, False)[3]
    lam, sigma, T = S.REFINE_LAMBDA, S.REFINE_SIGMA, S.REFINE_ITERS
    refined = R.refine(want["final"], conf, left, R.tables(lam, sigma, T, S.load_library()), False)
    i = sym_instance(7, 7, keep=False)
    try:
        assert i.set_refine(True, lam, sigma, T, False) and i.reset(w, h, opt)
        assert_same(i.match(left, right), refined, "refined map")
    finally:
        i.close()


def test_match_planes_depth_with_the_symmetric_census(oracle):
    import soc_project_stereo_matching_amd as S
    from oracle.platform_oracle import board_gray, disparity_to_depth
    w, h, d = 70, 33, 16
    fx, baseline, doffs = 1733.74, 536.62, 0.0
    opt = default_option(d, min_speckle_area=9)
    rng = np.random.default_rng(5)
    l, r = oracle.synth_pair(w, h, d, 0x91A5)
    planes = np.empty((6, h, w), np.uint8)
    for v, g in enumerate((l, r)):
        for c in range(3):
            planes[3 * v + c] = np.clip(g.astype(np.int32) + rng.integers(-6, 7, (h, w)), 0, 255)
    gl, gr = board_gray(planes[0], planes[1], planes[2]), board_gray(planes[3], planes[4], planes[5])
    disp = CS.pipeline(oracle, gl, gr, opt, 7, 7)["final"]
    want = disparity_to_depth(disp, fx, baseline, doffs)
    i = sym_instance(7, 7, keep=False)
    try:
        assert i.reset(w, h, opt)
        got = np.empty((h, w), np.float32)
        assert i.match_planes(planes, fx, baseline, doffs, got)
        assert_same(i.read_stage("final"), disp, "disparity behind the depth map")
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    finally:
        i.close()


def test_two_matches_without_reset_accumulate(oracle):
    w, h, d = 48, 20, 16
    opt = default_option(d, min_speckle_area=8)
    a, b = oracle.synth_pair(w, h, d, 0x0140), oracle.synth_pair(w, h, d, 0x0141)
    first = CS.pipeline(oracle, a[0], a[1], opt, 7, 7)
    second = CS.pipeline(oracle, b[0], b[1], opt, 7, 7, S_prev=first["aggr"])
    i = sym_instance(7, 7, keep=False)
    try:
        assert i.reset(w, h, opt)
        assert_same(i.match(a[0], a[1]), first["final"], "first")
        assert_same(i.match(b[0], b[1]), second["final"], "second (no reset)")
        assert_same(i.read_stage("aggr"), second["aggr"], "S after two frames")
    finally:
        i.close()


def test_three_row_tiles_in_one_process(oracle, monkeypatch):
    """Row tiles compute the census of the blocks their need map names, nothing else: with the buffers poisoned first, a
    word nobody computed cannot pass as stale data."""
    import torch
    import soc_project_stereo_matching_amd as S
    from soc_project_stereo_matching_amd.tiling import DeviceTileEngine, match_tiled_in_process, tile_rows
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")
    w, h, d = 200, 64, 48
    opt = default_option(d, min_speckle_area=12)
    left, right = oracle.synth_pair(w, h, d, 0x7A7)
    want = CS.pipeline(oracle, left, right, opt, 9, 7)
    engines = []
    try:
        for rows in tile_rows(h, 3):
            e = DeviceTileEngine.__new__(DeviceTileEngine)
            e.torch, e.dev = torch, torch.device("cuda", 0)
            e.w, e.h, e.rows, e.option = w, h, rows, opt
            e.inst = S.SGMInstance(0)
            engines.append(e)
            assert e.inst.set_census_kind(SYM) and e.inst.set_census_window(9, 7) and e.inst.set_rows(*rows) and e.inst.reset(w, h, opt)
            e.disp = torch.empty((h, w), dtype=torch.float32, device=e.dev)
            e.nbytes = e.inst.tile_boundary_bytes()
        got = match_tiled_in_process(engines, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
        assert_same(got.cpu().numpy(), want["final"], "three row tiles")
        for e in engines:
            r0, r1 = e.rows
            assert_same(e.inst.read_stage("aggr")[r0:r1], want["aggr"][r0:r1], f"S rows {r0}:{r1}")
    finally:
        for e in engines:
            e.inst.close()


def test_default_instance_keeps_the_kind_across_shutdown(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0xDEF)
    want = CS.pipeline(oracle, left, right, opt, 7, 7)
    g = S.SGM()
    g.shutdown()
    try:
        assert not g.set_census_kind(2)
        assert g.set_census_kind(SYM) and g.set_census_window(7, 7)
        assert g.reset(w, h, opt)
        g.keep_stages(True)
        assert_same(g.match(left, right), want["final"], "default instance")
        check_stages(g.read_stages(), want, "default instance")
        g.shutdown()                                                  # a new default instance: the kind and the window stay
        assert g.reset(w, h, opt)
        assert_same(g.match(left, right), want["final"], "default instance, re-created")
        assert g.read_stage("census_l").dtype == np.uint32
    finally:
        g.set_census_kind(0)
        g.set_census_window(5, 5)
        g.shutdown()
    assert g.reset(w, h, opt)
    assert_same(g.match(left, right), oracle.run(left, right, opt)["final"], "the reference's census again")
    g.shutdown()


def test_the_fast_path_is_taken(oracle):
    """Symmetric 9x7 against the centre 9x7 window of the materialised path, same frame.  Words: u32 against u64.  Cost volume:
    none (stage 2 reads 0 bytes without sgm_keep_stages) against a materialised one.  Timing: "cost" is empty on BOTH paths --
    the centre path's sgmd_cost64 runs inside its "census" interval, beside the window kernel -- so the contrast that can be
    asserted is the structural one; the "census" times of the two are printed (tools/census_sym_bench.py measures them)."""
    import soc_project_stereo_matching_amd as S
    w, h, d = 640, 480, 128
    opt = default_option(d)
    left, right = oracle.synth_pair(w, h, d, 0xFA57)
    timing = {}
    for kind in (SYM, 0):
        i = S.SGMInstance(0)
        try:
            assert i.set_census_kind(kind) and i.set_census_window(9, 7)
            i.enable_timing(True)
            for _ in range(3):
                assert i.reset(w, h, opt)
                assert i.match(left, right) is not None
            assert i.synchronize()
            timing[kind] = i.mean_timing()[1]                         # the minimum of the three matches
            print("census kind", kind, {k: round(v, 4) for k, v in timing[kind].items()})
            words = np.empty((h, w), np.uint64)
            n0 = i.lib.sgm_read_stage(i.handle, 0, words.ctypes.data, words.nbytes)
            cost = np.empty((h, w, d), np.uint8)
            n2 = i.lib.sgm_read_stage(i.handle, 2, cost.ctypes.data, cost.nbytes)
            if kind == SYM:
                assert n0 == 4 * w * h and n2 == 0
                assert_same(i.read_stage("census_l"), CS.census_sym(left, 9, 7), "census_l")
            else:
                assert n0 == 8 * w * h and n2 == w * h * d
        finally:
            i.close()
    # an empty interval between two event marks: a few microseconds of event latency at the most
    assert timing[SYM]["cost"] < 0.05 and timing[0]["cost"] < 0.05


def test_switching_back_restores_the_reference_census(oracle):
    import soc_project_stereo_matching_amd as S
    w, h, d = 70, 33, 16
    opt = default_option(d, min_speckle_area=9)
    left, right = oracle.synth_pair(w, h, d, 0x5717)
    i, fresh = sym_instance(9, 7), S.SGMInstance(0)
    try:
        fresh.keep_stages(True)
        assert i.reset(w, h, opt)
        assert_same(i.match(left, right), CS.pipeline(oracle, left, right, opt, 9, 7)["final"], "symmetric 9x7")
        assert i.set_census_kind(0) and i.set_census_window(5, 5)
        assert i.match(left, right) is None                           # the kind takes effect at the next initialize / reset
        assert i.reset(w, h, opt) and fresh.reset(w, h, opt)
        a, b = i.match(left, right), fresh.match(left, right)
        assert_same(a, b, "5x5 after symmetric")
        assert_same(a, oracle.run(left, right, opt)["final"], "5x5 against the oracle")
        got, want = i.read_stages(), fresh.read_stages()
        for n in STAGE_NAMES:
            assert_same(got[n], want[n], f"5x5 after symmetric:{n}")
    finally:
        i.close()
        fresh.close()
