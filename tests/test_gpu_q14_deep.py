"""Matches without Reset until the uint16 cost sums pass 15 bits and wrap (tests/q14_deep.py has the sequence and
the regime counters) on the device, against the CPU oracle fed the same sequence -- needs an MI355X.

What only this regime reaches: the accumulating (SLOW) variant of the fused cost-sum / WTA kernel with its per-half packed add,
the 32-bit accumulator of the separate sum kernel masked to 16 bits, the (int16) casts and the clamp of the parabola's
denominator in wta_finish, keys S << 16 | d with bit 31 set in both winner-take-all views, and the lazy materialisation of S
after a fast fused match (test_q14_deep_cpu.py shows that the sequences get there, and pins the oracle on the reference's own
hundred matches).  Every match's final map is compared, at the checkpoints of a sequence also S and the raw / LR-checked maps.
Tolerance: 0 everywhere, bit patterns; a mismatch names the first failing match and stage.

Penalties: with the default P1 / P2 only the cells left of the image (x - d < 0, constant cost) climb fast enough to wrap within a
hundred matches, and the right view never reads those; "interior" (P1 = P2 = 32767, 160 matches) lets the cells of real pixels
pass 32768 and wrap too, which brings the right view, and best costs >= 32768 in both views, into the regime."""
import json
import os

import numpy as np
import pytest

import confidence_ref
import q14_deep as Q
from conftest import GOLDEN
from oracle.pyoracle import sha

pytestmark = pytest.mark.gpu

# name -> (option overrides, matches N)
PENALTIES = {"default": ((), Q.N), "interior": ((("p1", 32767), ("p2_init", 32767)), 160)}

# one shape per instantiation of the sum kernels: padded stride Dp / 16 = 2, 4, 8 (D = 100: padding disparities inside the stride),
# 8, 12, 16, 32 (D > 256: always the separate kernels), and a W < H shape; (w, h, dmin, dmax).  N as in PENALTIES for every one:
# each has wrapped cells by match 48 (default) / 36 (interior); oracle_sequence() asserts that every sequence wraps
SHAPES = {"48x20_d16": (48, 20, 0, 16), "40x12_dmin3_d40": (40, 12, 3, 43), "64x10_d100": (64, 10, 0, 100),
          "64x10_d128": (64, 10, 0, 128), "56x8_d192": (56, 8, 0, 192), "48x8_d256": (48, 8, 0, 256), "72x6_d300": (72, 6, 0, 300),
          "14x30_d8": (14, 30, 0, 8)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={got[first]} oracle={want[first]}")


def oracle_sequence(shape, penalties="default", n=None, **kw):
    opt, n_default = PENALTIES[penalties]
    extra = tuple(sorted(kw.pop("opt", ())))
    s = Q.sequence(*shape, n=n or n_default, opt=tuple(sorted(opt + extra)), **kw)
    assert s.summary()["wrapped_cells"] > 0 and s.summary()["max_share15"] > 0, "the sequence never reaches the regime"
    return s


def new_instance(monkeypatch, fused=None, batch=1, **env):
    import soc_project_stereo_matching_amd as S
    if fused is not None:
        monkeypatch.setenv("SGM_FUSED_WTA", "1" if fused else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return S.SGMInstance(0, batch=batch)


def check_stages(inst, s, k, names, what):
    for name in names:
        assert_same(inst.read_stage(name), s.stages[k][name], f"{what}: match {k}: stage {name}")


def run_sequence(inst, s, what, stages=(), at="checkpoints", step=None, after_first=None):
    """Reset once, then s.n matches; every final map against the oracle's, `stages` at the checkpoints ("end": after the last
    match only).  step(inst, k, left, right) -> final map replaces the plain match."""
    w, h, _, _ = s.shape
    assert inst.reset(w, h, s.option)
    for k, (l, r) in enumerate(s.frames):
        out = step(inst, k, l, r) if step else inst.match(l, r)
        assert out is not None, f"{what}: match {k} returned false"
        if k == 0 and after_first:
            after_first(inst)
        assert_same(out, s.finals[k], f"{what}: match {k}: final map")
        if stages and (k in s.checkpoints if at == "checkpoints" else k == s.n - 1):
            check_stages(inst, s, k, stages, what)


# default: the fast fused kernel for match 0, then S materialised lazily and the accumulating variant without a store (a
#          read-back would change that, so stages are read after the last match only; two of them exist without keep_stages);
# keep:    keep_stages, the accumulating variant storing S throughout; separate: SGM_FUSED_WTA=0
MODES = {"default": dict(fused=True, keep=False, stages=("aggr", "disp_r"), at="end"),
         "keep": dict(fused=True, keep=True, stages=Q.Sequence.STAGES, at="checkpoints"),
         "separate": dict(fused=False, keep=True, stages=Q.Sequence.STAGES, at="checkpoints")}


@pytest.mark.parametrize("penalties", list(PENALTIES))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_sum_kernel_through_the_wrap(monkeypatch, shape, mode, penalties):
    m = MODES[mode]
    s = oracle_sequence(SHAPES[shape], penalties)
    inst = new_instance(monkeypatch, m["fused"])
    try:
        inst.keep_stages(m["keep"])
        run_sequence(inst, s, f"{shape} {mode} {penalties}", m["stages"], m["at"])
    finally:
        inst.close()


@pytest.mark.parametrize("penalties", list(PENALTIES))
def test_after_a_fused_last_sweep(monkeypatch, penalties):
    """SGM_UPSUM=1: match 0 runs the fused last sweep and leaves five planes; S for match 1 is put together from those and the
    three re-walked directions, and every later match adds to it."""
    s = oracle_sequence(SHAPES["64x10_d128"], penalties)
    inst = new_instance(monkeypatch, True, SGM_UPSUM=1)
    try:
        inst.keep_stages(False)
        rows = []
        run_sequence(inst, s, f"upsum {penalties}", ("aggr", "disp_r"), "end", after_first=lambda i: rows.append(i.fused_sweep_rows()))
        assert rows[0] > 0, "match 0 did not run the fused last sweep"
        assert inst.fused_sweep_rows() == 0
    finally:
        inst.close()


def test_after_a_match_in_row_segments(monkeypatch):
    """SGM_SUM_SEGMENTS=3 on a wide, low frame: match 0 sums every row in three overlapping segments (never when S is read or
    written); the S materialised for match 1 must not hold the overlaps twice."""
    # the launcher lowers the count while W / segments < 2 * Dp: D = 16 pads to Dp = 32, and 208 / 3 = 69 >= 64 keeps three
    # (seg_len = 80: segments of 80, 80 and 48 columns); H = 7 because a 5-row frame would make the 5x5 census a no-op
    s = oracle_sequence((208, 7, 0, 16), "interior")
    inst = new_instance(monkeypatch, True, SGM_SUM_SEGMENTS=3)
    try:
        inst.keep_stages(False)
        run_sequence(inst, s, "three segments", ("aggr", "disp_r"), "end")
    finally:
        inst.close()


@pytest.mark.parametrize("penalties", list(PENALTIES))
@pytest.mark.parametrize("mode", ["default", "keep"])
def test_batch_of_three(monkeypatch, mode, penalties):
    """Three frames per launch, each with a sequence (base) of its own, each against its own oracle context."""
    m = MODES[mode]
    shape = SHAPES["64x10_d100"]
    seqs = [oracle_sequence(shape, penalties, base=Q.BASE + 0x100 * j) for j in range(3)]
    w, h = shape[:2]
    inst = new_instance(monkeypatch, True, batch=3)
    try:
        inst.keep_stages(m["keep"])
        assert inst.reset(w, h, seqs[0].option)
        for k in range(seqs[0].n):
            out = inst.match(np.stack([s.frames[k][0] for s in seqs]), np.stack([s.frames[k][1] for s in seqs]))
            assert out is not None
            for j, s in enumerate(seqs):
                what = f"batch {mode} {penalties}: frame {j}"
                assert_same(out[j], s.finals[k], f"{what}: match {k}: final map")
                if k in s.checkpoints if m["at"] == "checkpoints" else k == s.n - 1:
                    inst.select_frame(j)
                    check_stages(inst, s, k, m["stages"], what)
    finally:
        inst.close()


@pytest.mark.parametrize("penalties", list(PENALTIES))
@pytest.mark.parametrize("right_view", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_confidence_on_accumulated_costs(monkeypatch, fused, right_view, penalties):
    """Every match through sgm_match_confidence: the disparity is the plain sequence's, the confidence is tests/confidence_ref.py
    on the oracle's accumulated S, for either reference view."""
    shape = SHAPES["40x12_dmin3_d40"]
    s = oracle_sequence(shape, penalties, right_view=right_view, keep_S=True)
    inst = new_instance(monkeypatch, fused)
    try:
        inst.set_reference_view(right_view)
        what = f"confidence fused={fused} right={right_view} {penalties}"

        def step(i, k, l, r):
            out, conf = i.match_confidence(l, r)
            assert_same(conf, confidence_ref.confidence(s.stages[k]["aggr"], shape[2], right_view)[3], f"{what}: match {k}: confidence")
            return out
        run_sequence(inst, s, what, step=step)
    finally:
        inst.close()


@pytest.mark.parametrize("penalties", list(PENALTIES))
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_both_views_on_accumulated_costs(monkeypatch, fused, penalties):
    """Every match through sgm_match_both: the left map is the plain sequence's, the right map that of an oracle context with
    the right image as the reference view fed the same sequence."""
    shape = SHAPES["48x20_d16"]
    s = oracle_sequence(shape, penalties)
    sr = oracle_sequence(shape, penalties, right_view=True)
    inst = new_instance(monkeypatch, fused)
    try:
        what = f"both views fused={fused} {penalties}"

        def step(i, k, l, r):
            out_l, out_r = i.match_both(l, r)
            assert_same(out_r, sr.finals[k], f"{what}: match {k}: right map")
            return out_l
        run_sequence(inst, s, what, step=step)
    finally:
        inst.close()


@pytest.mark.parametrize("penalties", list(PENALTIES))
def test_entry_points_by_turns(monkeypatch, penalties):
    """match, match_both, match_confidence by turns on the same S."""
    shape = SHAPES["40x12_dmin3_d40"]
    s = oracle_sequence(shape, penalties, keep_S=True)
    sr = oracle_sequence(shape, penalties, right_view=True, keep_S=True)
    inst = new_instance(monkeypatch, True)
    try:
        what = f"by turns {penalties}"

        def step(i, k, l, r):
            if k % 3 == 0:
                return i.match(l, r)
            if k % 3 == 1:
                out_l, out_r = i.match_both(l, r)
                assert_same(out_r, sr.finals[k], f"{what}: match {k}: right map of match_both")
                return out_l
            out, conf = i.match_confidence(l, r)
            assert_same(conf, confidence_ref.confidence(s.stages[k]["aggr"], shape[2], False)[3], f"{what}: match {k}: confidence")
            return out
        run_sequence(inst, s, what, ("aggr", "disp_r"), "end", step=step)
    finally:
        inst.close()


@pytest.mark.parametrize("penalties,n", [("default", 2 * Q.N), ("interior", 320)])
@pytest.mark.parametrize("mode", ["default", "separate"])
def test_four_paths(monkeypatch, mode, penalties, n):
    """SGM_SetHonorNumPaths(1) with num_paths = 4: a match adds at most 4 x 255 to a cell, so the sequences are twice as long."""
    m = MODES[mode]
    s = oracle_sequence(SHAPES["48x20_d16"], penalties, n=n, honor=True, opt=(("num_paths", 4),))
    inst = new_instance(monkeypatch, m["fused"])
    try:
        inst.set_honor_num_paths(True)
        inst.keep_stages(m["keep"])
        run_sequence(inst, s, f"four paths {mode} {penalties}", m["stages"], m["at"])
    finally:
        inst.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_census_7x7(monkeypatch, mode):
    """The wide-census path (materialised cost volume, volume-fed aggregation) feeding the same sums."""
    m = MODES[mode]
    s = oracle_sequence(SHAPES["48x20_d16"], "interior", window=(7, 7))
    inst = new_instance(monkeypatch, m["fused"])
    try:
        assert inst.set_census_window(7, 7)
        inst.keep_stages(m["keep"])
        run_sequence(inst, s, f"census 7x7 {mode}", m["stages"], m["at"])
    finally:
        inst.close()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_global_entry_points_against_the_reference(monkeypatch, fused):
    """SGM_Reset once, SGM_Match x 100 at 48x20 D = 16: every final map against the digests the compiled reference produced
    for the same calls (tests/golden/q14_deep.json), the maps at the checkpoints in full, and S at the end against the oracle."""
    import soc_project_stereo_matching_amd as S
    from conftest import load_npz
    name = "48x20_d16"
    with open(os.path.join(GOLDEN, "q14_deep.json")) as f:
        fx = json.load(f)["shapes"][name]
    maps = load_npz(f"q14_deep_{name}.npz")
    s = oracle_sequence(Q.FIXTURE_SHAPES[name])
    g = S.SGM()
    g.shutdown()                                                  # a new default instance: reads SGM_FUSED_WTA
    monkeypatch.setenv("SGM_FUSED_WTA", fused)
    try:
        assert g.reset(fx["w"], fx["h"], S.default_option(fx["dmax"], fx["dmin"], min_speckle_area=fx["min_speckle_area"]))
        for k, (l, r) in enumerate(s.frames):
            out = g.match(l, r)
            assert out is not None
            assert sha(out) == fx["matches"][k]["sha256"], f"SGM_Match {k} without Reset differs from the reference (fused={fused})"
            assert int(np.isinf(out).sum()) == fx["matches"][k]["invalid"]
            if f"final_{k}" in maps:
                assert_same(out, maps[f"final_{k}"], f"global entry points fused={fused}: match {k}: final map")
        assert_same(g.read_stage("aggr"), s.stages[s.n - 1]["aggr"], f"global entry points fused={fused}: S after {s.n} matches")
    finally:
        g.shutdown()
