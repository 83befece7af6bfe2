"""Every kernel at the limits sgm_initialize admits -- needs an MI355X.  The cases are those of tests/limits.py:

  A  min_disparity in the hundreds and up to 65535 - D: the right census base moved dmin + Dp words down into the zero-filled slack
     in front of the buffer, the fused sum's dmin + D - 1 iterations past the row end, the census need map of the row tiles;
  B  frames 65535 wide or tall: the 16-bit column tracker of the W <= H diagonal walk, column / slot pairs packed into 16 + 16
     bits, 256 chained median bands, one 524 280-pixel speckle component;
  C  padded cost volumes W * H * Dp between 2^31 and 2^32 cells: every 32-bit cell offset with bit 31 set;
  D  the ends of the option fields.

Bit-exact, tolerance 0, against the CPU oracle (parts A, B, D: test_limits_cpu.py pins the oracle on these very cases to the
reference's own C) and against the reference's digests (part C, tests/golden/limits.json).  NOTES.md has the wall times."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import limits as LM
from oracle.pyoracle import STAGE_NAMES, Oracle, default_option, sha
from test_gpu_instance_reuse import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"default": {}, "separate_sum": {"SGM_FUSED_WTA": "0"}, "plain_step": {"SGM_AGG_FAST": "0"}}
MAPS = ("disp_l", "disp_r", "after_lr", "after_speckle", "final")


def instance(monkeypatch, batch=1, **env):
    import soc_project_stereo_matching_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))                          # read at sgm_create / at the launch
    return S.SGMInstance(0, batch=batch)


def run_oracle(left, right, opt, view=False, honor=False, window=(5, 5), prev=None):
    """the nine stages by a context of its own (zeroed census words, its own S); prev: a pair matched before, without Reset"""
    orc = Oracle()
    orc.set_honor_num_paths(honor)
    assert orc.set_census_window(*window)
    orc.set_reference_view(view)
    h, w = left.shape
    assert orc.reset(w, h, opt)
    if prev is not None:
        assert orc.match(*prev) is not None
    assert orc.match(left, right) is not None
    return orc.stages()


def check_all_stages(inst, out, want, what):
    assert out is not None, what
    got = inst.read_stages()
    for n in STAGE_NAMES:
        assert_same(got[n], want[n], f"{what}: {n}")
    assert_same(out, want["final"], f"{what}: result")


def match_frames(inst, pairs):
    if len(pairs) == 1:
        out = inst.match(*pairs[0])
        return None if out is None else out[None]
    return inst.match(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))


# =============================================================================================== A. large minimum disparity

_dmin_cache = {}


def dmin_input(oracle, case, frame=0):
    """(left, right, the oracle's nine stages) of a case's frame: computed once, shared, left unchanged"""
    key = (tuple(case), frame)
    if key not in _dmin_cache:
        left, right = LM.dmin_pair(oracle.synth_pair, case, frame)
        st = run_oracle(left, right, LM.dmin_option(case))
        for a in (left, right) + tuple(st.values()):
            a.setflags(write=False)
        _dmin_cache[key] = (left, right, st)
    return _dmin_cache[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", LM.DMIN_CASES, ids=LM.dmin_name)
def test_large_min_disparity(oracle, monkeypatch, case, mode):
    left, right, want = dmin_input(oracle, case)
    if case in LM.DMIN_IN_RANGE:
        assert min(np.isfinite(want["final"]).sum(), np.isfinite(want["disp_r"]).sum()) >= LM.DMIN_QUOTA
    i = instance(monkeypatch, **MODES[mode])
    try:
        i.keep_stages(True)
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        check_all_stages(i, i.match(left, right), want, f"{LM.dmin_name(case)} {mode}")
    finally:
        i.close()


@pytest.mark.parametrize("case", LM.DMIN_CASES, ids=LM.dmin_name)
def test_large_min_disparity_in_a_batch(oracle, monkeypatch, case):
    """Three different frames, 8 lanes per pixel: frame f's masked census reads in front of its rows land in frame f - 1."""
    frames = [dmin_input(oracle, case, f) for f in range(3)]
    i = instance(monkeypatch, batch=3)
    try:
        i.keep_stages(True)
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        out = match_frames(i, [f[:2] for f in frames])
        assert out is not None
        for k, (_, _, want) in enumerate(frames):
            i.select_frame(k)
            check_all_stages(i, out[k], want, f"{LM.dmin_name(case)} frame {k} of 3")
    finally:
        i.close()


@pytest.mark.parametrize("segments", [1, 2, 3, 4])
@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_row_segments(oracle, monkeypatch, case, segments):
    """Segments of the fused sum kernel re-sum dmin + D - 1 columns of their right neighbour (stages off: only then are rows cut)."""
    left, right, want = dmin_input(oracle, case)
    i = instance(monkeypatch, SGM_SUM_SEGMENTS=segments, SGM_FUSED_WTA=1)
    try:
        i.keep_stages(False)
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        out = i.match(left, right)
        assert out is not None
        assert_same(i.read_stage("disp_r"), want["disp_r"], f"segments={segments}: right view")
        assert_same(out, want["final"], f"segments={segments}: final")
        assert_same(i.read_stage("aggr"), want["aggr"], f"segments={segments}: S (materialised afterwards)")
    finally:
        i.close()


@pytest.mark.parametrize("rows", [3, 1])
def test_large_min_disparity_fused_last_sweep(oracle, monkeypatch, rows):
    case = LM.DMIN_EXTRA[1]
    assert LM.padded_stride(case[3]) == 128
    left, right, want = dmin_input(oracle, case)
    i = instance(monkeypatch, SGM_UPSUM=1, SGM_UPSUM_ROWS=rows)
    try:
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        out = i.match(left, right)
        assert out is not None and i.fused_sweep_rows() == rows
        assert_same(i.read_stage("disp_r"), want["disp_r"], f"rows={rows}: right view")
        assert_same(out, want["final"], f"rows={rows}: final")
        assert_same(i.read_stage("aggr"), want["aggr"], f"rows={rows}: S after the fact")
    finally:
        i.close()


@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_four_paths(oracle, monkeypatch, case):
    left, right, _ = dmin_input(oracle, case)
    opt = LM.dmin_option(case, num_paths=4)
    want = run_oracle(left, right, opt, honor=True)
    i = instance(monkeypatch)
    try:
        i.set_honor_num_paths(True)
        i.keep_stages(True)
        assert i.reset(case[0], case[1], opt)
        check_all_stages(i, i.match(left, right), want, "four paths")
    finally:
        i.close()


@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_right_view_and_both(oracle, monkeypatch, case):
    left, right, want_l = dmin_input(oracle, case)
    opt = LM.dmin_option(case)
    want_r = run_oracle(left, right, opt, view=True)
    i = instance(monkeypatch)
    try:
        i.keep_stages(False)
        assert i.reset(case[0], case[1], opt)
        both = i.match_both(left, right)
        assert both is not None
        assert_same(both[0], want_l["final"], "both: left")
        assert_same(both[1], want_r["final"], "both: right")
        i.set_reference_view(True)
        i.keep_stages(True)
        assert i.reset(case[0], case[1], opt)
        check_all_stages(i, i.match(left, right), want_r, "right reference view")
    finally:
        i.close()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_confidence(oracle, monkeypatch, case, fused):
    import confidence_ref as CR
    left, right, want = dmin_input(oracle, case)
    opt = LM.dmin_option(case)
    i = instance(monkeypatch, SGM_FUSED_WTA=fused)
    try:
        i.keep_stages(False)
        for view in (False, True):
            i.set_reference_view(view)
            assert i.reset(case[0], case[1], opt)
            got = i.match_confidence(left, right)
            assert got is not None
            assert_same(got[0], (run_oracle(left, right, opt, view=True) if view else want)["final"], f"view {view}: map")
            assert_same(got[1], CR.confidence(want["aggr"], case[2], view)[3], f"view {view}: confidence")
    finally:
        i.close()


@pytest.mark.parametrize("kind,window", [(1, (7, 7)), (0, (9, 7))], ids=["symmetric7x7", "centre9x7"])
@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_census_kinds(oracle, monkeypatch, case, kind, window):
    """The symmetric census (the u32 words of the fast path) and the centre 9x7 window (u64 words, sgm_cost64_k: the aggregation
    fed from a cost volume)."""
    import census_sym_ref as CS
    left, right, _ = dmin_input(oracle, case)
    opt = LM.dmin_option(case)
    want = CS.pipeline(oracle, left, right, opt, *window) if kind == 1 else run_oracle(left, right, opt, window=window)
    i = instance(monkeypatch)
    try:
        assert i.set_census_kind(kind) and i.set_census_window(*window)
        i.keep_stages(True)
        assert i.reset(case[0], case[1], opt)
        out = i.match(left, right)
        assert out is not None
        assert_same(out, want["final"], "result")
        for n in ("cost", "aggr") + MAPS:
            assert_same(i.read_stage(n), want[n], n)
    finally:
        i.close()


@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_hole_filling(oracle, monkeypatch, case):
    import fill_holes_ref as FH
    left, right, want = dmin_input(oracle, case)
    opt = LM.dmin_option(case)
    cls, filled, final = FH.expected(want, opt, oracle)
    i = instance(monkeypatch)
    try:
        i.keep_stages(True)
        assert i.set_fill_holes(True) and i.reset(case[0], case[1], opt)
        out = i.match(left, right)
        assert out is not None
        assert_same(i.read_stage("after_speckle"), want["after_speckle"], "stage 7")
        assert_same(i.read_fill_classes(), cls, "classes")
        assert_same(i.read_filled(), filled, "filled")
        assert_same(out, final, "final")
    finally:
        i.close()


@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_12_bit_pixels(oracle, monkeypatch, case):
    """v = u8 << 4: the census compares the same, the narrowed guide is the u8 image: the oracle's result on the 8-bit pair."""
    left, right, want = dmin_input(oracle, case)
    i = instance(monkeypatch)
    try:
        assert i.set_pixel_bits(12)
        i.keep_stages(True)
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        out = i.match(left.astype(np.uint16) << 4, right.astype(np.uint16) << 4)
        assert out is not None
        assert_same(out, want["final"], "result")
        for n in ("aggr",) + MAPS:
            assert_same(i.read_stage(n), want[n], n)
    finally:
        i.close()


@pytest.mark.parametrize("mode", ["fused", "fused_keep", "separate"])
@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_second_match_without_reset(oracle, monkeypatch, case, mode):
    a, b = dmin_input(oracle, case, 0), dmin_input(oracle, case, 1)
    opt = LM.dmin_option(case)
    want = run_oracle(b[0], b[1], opt, prev=a[:2])
    i = instance(monkeypatch, SGM_FUSED_WTA=0 if mode == "separate" else 1)
    try:
        i.keep_stages(mode != "fused")
        assert i.reset(case[0], case[1], opt)
        assert_same(i.match(a[0], a[1]), a[2]["final"], f"{mode}: first")
        assert_same(i.match(b[0], b[1]), want["final"], f"{mode}: second (no reset)")
        for n in (("disp_r", "aggr") if mode == "fused" else MAPS + ("aggr",)):
            assert_same(i.read_stage(n), want[n], f"{mode}: second: {n}")
    finally:
        i.close()


def tile_engines(w, h, opt, n):
    import torch
    import soc_project_stereo_matching_amd as S
    from soc_project_stereo_matching_amd.tiling import DeviceTileEngine, tile_rows
    engines = []
    for rows in tile_rows(h, n):
        e = DeviceTileEngine.__new__(DeviceTileEngine)           # (as DeviceTileEngine(0, w, h, opt, rows); closed by the caller even
        e.torch, e.dev = torch, torch.device("cuda", 0)          # where a later engine's reset fails)
        e.w, e.h, e.rows, e.option = w, h, rows, opt
        e.inst = S.SGMInstance(0)
        engines.append(e)
        assert e.inst.set_rows(*rows) and e.inst.reset(w, h, opt)
        e.disp = torch.empty((h, w), dtype=torch.float32, device=e.dev)
        e.nbytes = e.inst.tile_boundary_bytes()
    return engines


@pytest.mark.parametrize("case", LM.DMIN_EXTRA, ids=LM.dmin_name)
def test_large_min_disparity_three_row_tiles(oracle, monkeypatch, case):
    """The census need map of a row tile depends on dmin + D; a census word nobody computed is poisoned, not stale."""
    import torch
    from soc_project_stereo_matching_amd.tiling import match_tiled_in_process
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")
    left, right, want = dmin_input(oracle, case)
    engines = []
    try:
        engines = tile_engines(case[0], case[1], LM.dmin_option(case), 3)
        got = match_tiled_in_process(engines, torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda())
        assert_same(got.cpu().numpy(), want["final"], "three row tiles")
        for e in engines:
            r0, r1 = e.rows
            assert_same(e.inst.read_stage("aggr")[r0:r1], want["aggr"][r0:r1], f"S rows {r0}:{r1}")
    finally:
        for e in engines:
            e.inst.close()


# =============================================================================================== B. frames 65535 wide or tall

def wide_modes(case):
    return list(MODES) if case[0] < case[1] else ["default", "separate_sum"]


@pytest.mark.parametrize("case,mode", [(c, m) for c in LM.WIDE_CASES for m in wide_modes(c)],
                         ids=lambda v: LM.wide_name(v) if isinstance(v, tuple) else v)
def test_wide_and_tall_frames(oracle, monkeypatch, case, mode):
    w, h, dmin, d, batch = case
    opt = LM.wide_option(case)
    pairs = [LM.wide_pair(oracle.synth_pair, case, f) for f in range(batch)]
    i = instance(monkeypatch, batch=batch, **MODES[mode])
    try:
        i.keep_stages(True)
        assert i.reset(w, h, opt)
        out = match_frames(i, pairs)
        assert out is not None
        for k, (l, r) in enumerate(pairs):
            i.select_frame(k)
            check_all_stages(i, out[k], oracle.run(l, r, opt), f"{LM.wide_name(case)} {mode} frame {k}")
    finally:
        i.close()


def test_widest_frame_fused_last_sweep(oracle, monkeypatch):
    case = (65535, 5, 0, 128, 1)
    assert case in LM.WIDE_CASES
    opt = LM.wide_option(case)
    left, right = LM.wide_pair(oracle.synth_pair, case)
    want = oracle.run(left, right, opt)
    i = instance(monkeypatch, SGM_UPSUM=1)
    try:
        assert i.reset(case[0], case[1], opt)
        out = i.match(left, right)
        assert out is not None and i.fused_sweep_rows() == 3
        assert_same(i.read_stage("disp_r"), want["disp_r"], "right view")
        assert_same(out, want["final"], "final")
        assert_same(i.read_stage("aggr"), want["aggr"], "S after the fact")
    finally:
        i.close()


def post_maps(w, h):
    from test_gpu_parity import _speckle_maps
    maps = _speckle_maps(np.random.default_rng(w * 1000 + h), h, w)
    return {n: maps[n] for n in LM.POST_MAPS}


def check_post(inst, oracle, w, h, areas, what, twice=False):
    """crafted maps through the whole-frame post entry against the oracle's speckle removal + median"""
    import torch
    import soc_project_stereo_matching_amd as S
    maps = post_maps(w, h)
    for area in areas:
        assert inst.reset(w, h, S.default_option(16, min_speckle_area=area))
        for name, m in maps.items():
            want = oracle.median(oracle.remove_speckles(m, area))
            for rep in range(2 if twice else 1):
                t = torch.from_numpy(m.copy()).cuda()
                torch.cuda.synchronize()
                assert inst.tile_post(t.data_ptr()) and inst.synchronize()
                assert_same(t.cpu().numpy(), want, f"{what} {name} {w}x{h} min_area={area} visit {rep}")


@pytest.mark.parametrize("tile_rows", [16, 64])
@pytest.mark.parametrize("shape", LM.POST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_post_filters_on_the_widest_and_tallest_maps(oracle, monkeypatch, shape, tile_rows):
    """`flat` is one component of 524 280 pixels; the tall map is 256 chained median bands."""
    i = instance(monkeypatch, SGM_SPECKLE_TILE_ROWS=tile_rows)
    try:
        check_post(i, oracle, shape[0], shape[1], LM.POST_AREAS, f"tile rows {tile_rows}")
    finally:
        i.close()


def _median_chain_child(chain):
    """SGM_MEDIAN_CHAIN is read once per process, at the first median launch: the tall maps in a process of their own"""
    import soc_project_stereo_matching_amd as S
    assert os.environ["SGM_MEDIAN_CHAIN"] == chain
    w, h = LM.POST_SHAPES[1]
    i = S.SGMInstance(0)
    try:
        check_post(i, Oracle(), w, h, (50,), f"chain={chain}", twice=True)
    finally:
        i.close()
    print("median chain child ok")


@pytest.mark.parametrize("chain", ["1", "0"])
def test_median_chain_on_and_off_on_the_tallest_map(chain):
    env = dict(os.environ, SGM_MEDIAN_CHAIN=chain,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "median_chain", chain], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "median chain child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ============================================================================ C. volumes with bit 31 set in the cell offset

def big_case(name):
    from conftest import option_from_dict
    import soc_project_stereo_matching_amd as S
    c = LM.golden()["big"][name]
    left, right = S.synth_pair(c["w"], c["h"], c["d"], c["seed"])
    assert sha(left) == c["sha256_inputs"]["left"] and sha(right) == c["sha256_inputs"]["right"]
    return c, left, right, option_from_dict(c["option"])


@pytest.mark.parametrize("name", list(LM.BIG_CASES))
def test_volumes_past_2_31_cells(name):
    """Digests the REFERENCE produced for every stage (minutes of CPU time per case: make_golden_limits.py --big)."""
    import soc_project_stereo_matching_amd as S
    c, left, right, opt = big_case(name)
    i = S.SGMInstance(0)
    try:
        i.keep_stages(True)
        assert i.reset(c["w"], c["h"], opt)
        out = i.match(left, right)
        assert out is not None
        assert sha(out) == c["sha256"]["final"], "final"
        assert int(np.isinf(out).sum()) == c["invalid_final"]
        for n in STAGE_NAMES[:-1]:
            if n in ("cost", "aggr") and name not in LM.BIG_ALL_STAGES:
                continue
            if n == "cost" and name in LM.BIG_WITHOUT_COST:
                continue
            got = i.read_stage(n)
            assert sha(got) == c["sha256"][n], n
            if n == "aggr":
                assert int(got.max()) == c["aggr_max"] and int(got.sum(dtype=np.uint64)) == c["aggr_sum"]
            del got
            gc.collect()
    finally:
        i.close()
        gc.collect()


@pytest.mark.parametrize("name,rows", [("dp128_wide", 3), ("dp128_tall", 0)])
def test_volumes_past_2_31_cells_fused_last_sweep(monkeypatch, name, rows):
    """A second instance, stages off, SGM_UPSUM=1: the wide case runs the fused sweep, the tall one (W < H) is not eligible."""
    c, left, right, opt = big_case(name)
    i = instance(monkeypatch, SGM_UPSUM=1)
    try:
        i.keep_stages(False)
        assert i.reset(c["w"], c["h"], opt)
        out = i.match(left, right)
        assert out is not None and i.fused_sweep_rows() == rows
        assert sha(out) == c["sha256"]["final"], "final"
        assert sha(i.read_stage("disp_r")) == c["sha256"]["disp_r"], "right view"
    finally:
        i.close()
        gc.collect()


def test_volume_past_2_31_cells_as_two_row_tiles():
    """dp512 as two row tiles in one process: the size_t row offset of the plane copies, the boundary hand-overs."""
    import torch
    from soc_project_stereo_matching_amd.tiling import match_tiled_in_process
    c, left, right, opt = big_case("dp512")
    engines = []
    try:
        engines = tile_engines(c["w"], c["h"], opt, 2)
        got = match_tiled_in_process(engines, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
        assert sha(got.cpu().numpy()) == c["sha256"]["final"]
    finally:
        for e in engines:
            e.inst.close()
        gc.collect()


@pytest.mark.parametrize("w,h,d,accepted", LM.REFUSALS)
def test_refusal_boundary(w, h, d, accepted):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    try:
        assert bool(i.reset(w, h, default_option(d))) == accepted
    finally:
        i.close()
        gc.collect()


# =================================================================================================== D. ends of the option fields

@pytest.mark.parametrize("mode", ["default", "separate_sum"])
@pytest.mark.parametrize("name", list(LM.OPTION_ENDS))
def test_ends_of_the_option_fields(oracle, monkeypatch, name, mode):
    kw, honor, _ = LM.OPTION_ENDS[name]
    left, right = LM.option_pair(oracle.synth_pair)
    opt = LM.option_of(name)
    want = run_oracle(left, right, opt, honor=honor)
    i = instance(monkeypatch, **MODES[mode])
    try:
        i.set_honor_num_paths(honor)
        i.keep_stages(True)
        assert i.reset(LM.OPTION_SHAPE[0], LM.OPTION_SHAPE[1], opt)
        check_all_stages(i, i.match(left, right), want, f"{name} {mode}")
    finally:
        i.close()


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "median_chain":
    _median_chain_child(sys.argv[2])
