"""The CPU oracle at the limits sgm_initialize admits (tests/limits.py), against digests the reference's own C produced for these
very cases (tests/golden/limits.json, made by tests/golden/make_golden_limits.py): min_disparity up to 65535 - D, frames 65535
wide or tall, the ends of the option fields.  Nothing here needs the reference.  What the GPU tests of tests/test_gpu_limits.py
compare the library with is therefore the reference's result -- with one exception, pinned below: past 32768 columns or rows the
reference's RemoveSpeckles cuts components (int16_t neighbour coordinates), the oracle and the library keep them whole."""
import numpy as np
import pytest

import limits as LM
from oracle.pyoracle import STAGE_NAMES, Oracle, sha


def _check(got, frame, what):
    for n in STAGE_NAMES:
        assert sha(got[n]) == frame["sha256"][n], f"{what}: stage {n} differs from the reference"


@pytest.mark.parametrize("case", LM.DMIN_CASES, ids=LM.dmin_name)
def test_large_min_disparity(oracle, case):
    """Planted pairs (the true disparity sits at both ends of [dmin, dmin + D), in its middle and on a 16-lane boundary), three
    frames per case as the GPU test's batch has.  In range, both views hold at least DMIN_QUOTA finite pixels: a condition on the
    inputs.  From dmin + D > W on, columns leave the image; from dmin >= W everything is invalid by arithmetic."""
    want = LM.golden_case(LM.dmin_name(case))
    opt = LM.dmin_option(case)
    for f, frame in enumerate(want["frames"]):
        left, right = LM.dmin_pair(oracle.synth_pair, case, f)
        assert sha(left) == frame["sha256_inputs"]["left"] and sha(right) == frame["sha256_inputs"]["right"]
        got = oracle.run(left, right, opt)
        _check(got, frame, f"{LM.dmin_name(case)} frame {f}")
        finite = int(np.isfinite(got["final"]).sum()), int(np.isfinite(got["disp_r"]).sum())
        assert finite == (frame["finite_final"], frame["finite_disp_r"])
        if case in LM.DMIN_IN_RANGE:
            assert min(finite) >= LM.DMIN_QUOTA, finite
        if case[2] >= case[0]:
            assert finite == (0, 0) and (got["cost"] > 0).any() and (got["aggr"] > 0).any()


_kept = {}


def _wide(case, f):
    """the oracle's stages of a wide case's frame; only the two maps the int16-rule test needs are kept, and only for its cases"""
    orc = Oracle()
    st = orc.run(*LM.wide_pair(orc.synth_pair, case, f), LM.wide_option(case))
    if case in LM.INT16_RULE_CASES and f == 0:
        _kept[case] = {n: st[n] for n in ("after_lr", "after_speckle")}
    return st


def _maps(case):
    if case not in _kept:
        _wide(case, 0)
    return _kept[case]


@pytest.mark.parametrize("case", LM.WIDE_CASES, ids=LM.wide_name)
def test_wide_and_tall_frames(oracle, case):
    """Through after_lr the digests are the reference's at every size.  after_speckle and final are the reference's where W, H <=
    32768; beyond, they are the oracle's own (the generator stores the reference's beside them: the next test)."""
    want = LM.golden_case(LM.wide_name(case))
    assert want["equal_to_reference_through"] == ("after_lr" if LM.beyond_int16(case[0], case[1]) else "final")
    for f, frame in enumerate(want["frames"]):
        assert ("reference_sha256" in frame) == LM.beyond_int16(case[0], case[1])
        left, right = LM.wide_pair(oracle.synth_pair, case, f)
        assert sha(left) == frame["sha256_inputs"]["left"] and sha(right) == frame["sha256_inputs"]["right"]
        _check(_wide(case, f), frame, f"{LM.wide_name(case)} frame {f}")


@pytest.mark.parametrize("case", LM.INT16_RULE_CASES, ids=LM.wide_name)
def test_the_only_difference_to_the_reference_is_its_int16_neighbour_rule(oracle, case):
    """limits.reference_speckles -- the reference's RemoveSpeckles with its int16_t neighbour coordinates restated in Python --
    applied to the ORACLE's after_lr map gives the REFERENCE's after_speckle, and the oracle's median of that the reference's
    final: past 32768 columns / rows the two differ in that cut and in nothing else."""
    want = LM.golden_case(LM.wide_name(case))
    opt = LM.wide_option(case)
    for frame in want["frames"][:1]:                            # (one frame of a batch: each takes seconds in Python)
        st = _maps(case)
        cut = LM.reference_speckles(st["after_lr"], opt.min_speckle_area)
        assert sha(cut) == frame["reference_sha256"]["after_speckle"]
        assert sha(oracle.median(cut)) == frame["reference_sha256"]["final"]
        differ = int((cut.view(np.uint32) != st["after_speckle"].view(np.uint32)).sum())
        assert differ == frame["differ_from_reference"]["after_speckle"]
        # the cut only ever removes: what the reference keeps, the whole-component rule keeps as well
        assert not (np.isfinite(cut) & np.isinf(st["after_speckle"])).any()


def test_the_restated_rule_is_the_plain_one_up_to_32768(oracle):
    """Where no coordinate passes 32767 the restatement is the oracle's 8-connected rule: crafted and random maps."""
    rng = np.random.default_rng(0x5BEC)
    for (w, h) in [(64, 16), (33, 65), (200, 9)]:
        for k in range(3):
            m = (rng.integers(0, 6, (h, w)) * np.float32(0.75)).astype(np.float32)
            m[rng.random((h, w)) < 0.25] = np.inf
            for area in (1, 7, 50, 65535):
                assert np.array_equal(LM.reference_speckles(m, area).view(np.uint32),
                                      oracle.remove_speckles(m, area).view(np.uint32)), (w, h, k, area)


def test_the_restated_rule_on_a_crafted_map():
    """One row group across column 32767 | 32768: a flat run is cut there.  Its low part survives by its own size, every pixel
    beyond stands alone (area 1); only the pixel in column 32768 still looks back, into a component already taken."""
    m = np.full((3, 32780), np.inf, np.float32)
    m[1, 32700:32780] = 5.0
    out = LM.reference_speckles(m, 10)
    assert np.isfinite(out[1, 32700:32768]).all() and np.isinf(out[1, 32768:]).all()
    assert np.isfinite(LM.reference_speckles(m, 1)).sum() == 80
    # a component of min_area - 1 pixels in the low part that only a seed in column 32768 of the row above reaches first
    m = np.full((3, 32780), np.inf, np.float32)
    m[1, 32759:32768] = 5.0                                      # 9 pixels in row 1
    m[0, 32768] = 5.5                                            # the seed: row 0, raster order puts it in front of them
    out = LM.reference_speckles(m, 10)
    assert np.isfinite(out[1, 32759:32768]).all() and np.isfinite(out[0, 32768])      # 10 together
    m[0, 32768] = np.inf
    assert np.isinf(LM.reference_speckles(m, 10)).all()


@pytest.mark.parametrize("name", list(LM.OPTION_ENDS))
def test_ends_of_the_option_fields(oracle, name):
    want = LM.golden_case("option_" + name)
    kw, honor, by_reference = LM.OPTION_ENDS[name]
    assert want["by"] == ("reference" if by_reference else "oracle") and (name in LM.ORACLE_ONLY) == (not by_reference)
    assert want["note"] == LM.OPTION_NOTES.get(name, "")
    left, right = LM.option_pair(oracle.synth_pair)
    orc = Oracle()
    orc.set_honor_num_paths(honor)
    _check(orc.run(left, right, LM.option_of(name)), want["frames"][0], name)


def test_what_the_big_cases_reach():
    """Part C's fixtures (minutes of CPU time each: `make_golden_limits.py --big`): every padded volume has cells past 2^31 and
    stays below 2^32, every real volume fits the reference's int index, and the reference and the oracle agreed on them."""
    big = LM.golden()["big"]
    assert set(big) == set(LM.BIG_CASES)
    for name, (w, h, d, seed) in LM.BIG_CASES.items():
        c = big[name]
        assert (c["w"], c["h"], c["d"], c["seed"]) == (w, h, d, seed)
        assert c["padded_cells"] == w * h * LM.padded_stride(d) and 2 ** 31 < c["padded_cells"] < 2 ** 32 - 1
        assert c["real_cells"] == w * h * d < 2 ** 31
        assert set(c["sha256"]) == set(STAGE_NAMES)
    assert LM.golden()["oracle_only"] == LM.ORACLE_ONLY


def test_refusal_boundary_on_the_stand_in_device(tmp_path):
    """What sgm_initialize refuses, decided on the host before anything is allocated (the product's C host on the stand-in device
    of tests/standin.py): 2^32 padded cells, D = 513, 65535 x 65535, and a frame one pixel wide taller than 4096 rows -- there a
    diagonal step is W - 1 = 0 pixels, the anomalous lines stay on row 1 and the [H][cap] table of their visits has H x H (H even) or
    H x (H + 1) (H odd) entries, 2^24 at the most.  The cases the GPU test accepts with large volumes are left to it."""
    import ctypes as C
    import standin
    from oracle.pyoracle import default_option
    L = standin.build(tmp_path)
    s = L.sgm_create(0)
    try:
        for (w, h, d, accepted) in LM.REFUSALS:
            if accepted and w * h * LM.padded_stride(d) > 2 ** 26:
                continue
            opt = default_option(d)
            assert bool(L.sgm_reset(s, w, h, C.byref(opt))) == accepted, (w, h, d)
        opt = default_option(8)
        assert L.sgm_reset(s, 64, 20, C.byref(opt))                # and the instance is usable after a refusal
    finally:
        L.sgm_destroy(s)
