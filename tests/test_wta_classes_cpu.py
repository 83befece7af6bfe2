"""The planted winner-take-all inputs (tests/wta_classes.py) on the CPU: the oracle equals the reference's own C on them stage
by stage (digests in tests/golden/wta_classes.json, made by tests/golden/make_golden_wta_classes.py), the classifier's
restatement of the finish equals oracle.wta bit for bit in both views, and every class an input is meant to plant is taken by at
least 50 pixels or 1 % of the frame -- counted from the oracle's S, never from the library.

Excused, by the arithmetic and not by the choice of inputs:
  left view   none, edge_cost   no cell of S is 65535 after one match (a cell gains at most some 9 x 255 per match)
  left view   flat              in ONE match: d1 is the FIRST minimum, so S[d1 - 1] > m1 and S[d1 + 1] >= m1 and the denominator is
                                >= 1 until the (int16) casts bite at 32768.  The Q14 inputs (tests/q14_deep.py's sequences, some
                                sixty matches without Reset) get S there and plant it
  tie_far                       needs D > 16: at stride 32 the D = 32 input plants it"""
import functools
import json
import os

import numpy as np
import pytest

import wta_classes as WC
from conftest import GOLDEN
from oracle.pyoracle import STAGE_NAMES, sha

NAMES = [f"{s}-{v}" for s, v, _ in WC.INPUTS]
BY_NAME = {f"{s}-{v}": (s, v, seed) for s, v, seed in WC.INPUTS}

# padded disparity stride of the device kernels -> what some input of that stride has to plant, per view: every class but
# the excused ones, at every stride
LEFT = set(WC.CLASSES) - {"flat", "edge_cost", "none"}
REQUIRED = {dp: {"left": LEFT, "right": set(WC.CLASSES)} for dp in (32, 64, 128, 192, 256, 512)}
Q14_REQUIRED = {"q14-48x20_d16": {"left": {"flat", "first"}}, "q14-96x24_d48-interior": {"left": {"flat", "first"}, "right": {"flat"}}}


def stride(D):
    return next(dp for dp in (32, 64, 128, 192, 256, 512) if D <= dp)


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLDEN, "wta_classes.json")) as f:
        return json.load(f)["inputs"]


def test_the_fixture_lists_these_inputs():
    assert sorted(golden()) == sorted(NAMES + list(WC.Q14_INPUTS))


def test_every_listed_band_is_planted_at_every_range():
    """the issue's shapes carry the whole list of band disparities, over one or two inputs"""
    for shape in WC.ISSUE_SHAPES:
        _, _, dmin, dmax = WC.SHAPES[shape]
        planted = [k for s, v, seed in WC.INPUTS if s == shape and v in ("bands", "bands2") for k in WC.planted(s, v, seed).ks]
        D = dmax - dmin
        want = {0, 1, D - 2, D - 1, D, 15, 16, D // 2} | ({k for k in (63, 64, 127, 128, 255, 256) if k < D} if D > 64 else set())
        assert set(planted) == want, shape


@pytest.mark.parametrize("name", list(WC.Q14_INPUTS))
def test_q14_inputs(oracle, name):
    """matches without Reset: the oracle's final map equals the reference's after the same calls; the classifier's finish equals
    oracle.wta on the accumulated S; the left view takes the clamp on more pixels than the floor"""
    p, want = WC.q14_planted(name), golden()[name]
    w, h, dmin, dmax = p.shape
    assert want["matches"] == p.n and want["shape"] == list(p.shape) and want["options"] == p.option_kw
    assert sha(p.frames[-1][0]) == want["sha256_inputs"]["left"] and sha(p.frames[-1][1]) == want["sha256_inputs"]["right"]
    for n in WC.Q14_STAGES + ("final",):
        assert sha(p.stages[n]) == want["oracle_stages"][n], f"{name}: the oracle's stage {n} changed"
    assert want["reference_stages"]["final"] == want["oracle_stages"]["final"], f"{name}: oracle != reference"
    r, S = p.classify(), np.ascontiguousarray(p.stages["aggr"])
    for view, stage in (("left", "disp_l"), ("right", "disp_r")):
        ref = oracle.wta(S, dmin, dmax, True, p.option.uniqueness_ratio, view == "right")
        assert np.array_equal(r[view]["disp"].view(np.uint32), ref.view(np.uint32)), f"{name}: {view} view"
        assert np.array_equal(p.stages[stage].view(np.uint32), ref.view(np.uint32)), f"{name}: stage {stage}"
    got = p.counts()
    for view in WC.VIEWS:
        print(name, view, got[view])
        assert got[view] == want["counts"][view]
        for n in Q14_REQUIRED[name].get(view, ()):
            assert got[view][n] >= want["floor"] == WC.floor(w, h), f"{name}: {view} view: class {n}: {got[view][n]}"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_reference_digests(name):
    p, want = WC.planted(*BY_NAME[name]), golden()[name]
    assert want["seed"] == p.seed and want["shape"] == list(p.shape) and want["options"] == p.option_kw and want["bands"] == p.ks
    assert sha(p.left) == want["sha256_inputs"]["left"] and sha(p.right) == want["sha256_inputs"]["right"]
    for n in STAGE_NAMES:
        assert sha(p.stages[n]) == want["oracle_stages"][n], f"{name}: the oracle's stage {n} changed"
    o = p.option
    assert want["oracle_only"] == bool(o.min_disparity > 0 and o.is_check_lr and not o.is_check_unique)
    if want["oracle_only"]:
        assert want["reference_stages"] is None
    else:
        for n in STAGE_NAMES:
            assert want["reference_stages"][n] == want["oracle_stages"][n], f"{name}: stage {n}: oracle != reference"


@pytest.mark.parametrize("name", NAMES)
def test_classifier_finish_equals_oracle_wta(oracle, name):
    p = WC.planted(*BY_NAME[name])
    _, _, dmin, dmax = p.shape
    r = p.classify()
    S = np.ascontiguousarray(p.stages["aggr"])
    for view, stage in (("left", "disp_l"), ("right", "disp_r")):
        want = oracle.wta(S, dmin, dmax, p.unique, p.option.uniqueness_ratio, view == "right")
        assert np.array_equal(r[view]["disp"].view(np.uint32), want.view(np.uint32)), f"{name}: {view} view"
        assert np.array_equal(p.stages[stage].view(np.uint32), want.view(np.uint32)), f"{name}: stage {stage}"
        c = r[view]["classes"]
        assert not (c["none"] & np.isfinite(want)).any() and not (c["first"] & np.isfinite(want)).any()
        assert not (c["last"] & np.isfinite(want)).any()


@pytest.mark.parametrize("name", NAMES)
def test_quotas(name):
    p, want = WC.planted(*BY_NAME[name]), golden()[name]
    w, h = p.shape[:2]
    got = p.counts()
    assert want["floor"] == WC.floor(w, h) == max(50, -(-w * h // 100))
    for view in WC.VIEWS:
        print(name, view, got[view])
        assert got[view] == want["counts"][view], f"{name}: {view} view: class counts changed"
        for n in want["planted"][view]:
            assert got[view][n] >= want["floor"], f"{name}: {view} view: class {n}: {got[view][n]} pixels, floor {want['floor']}"
        assert want["planted"][view] == [n for n in WC.CLASSES if got[view][n] >= want["floor"]]


def test_every_stride_plants_every_class():
    have = {dp: {v: set() for v in WC.VIEWS} for dp in REQUIRED}
    for name, e in golden().items():
        if name in WC.Q14_INPUTS:
            continue
        dp = stride(e["shape"][3] - e["shape"][2])
        for v in WC.VIEWS:
            have[dp][v] |= set(e["planted"][v])
    for dp, views in REQUIRED.items():
        for v, need in views.items():
            assert need <= have[dp][v], f"stride {dp}, {v} view: nobody plants {sorted(need - have[dp][v])}"


def test_classifier_on_a_hand_made_volume():
    """One pixel per class, by hand: D = 20, dmin = 0, uniqueness on, ratio 0.99."""
    D = 20
    S = np.full((1, 8, D), 1000, np.uint16)
    S[0, 0, 0] = 10                                  # first
    S[0, 1, D - 1] = 10                              # last (and last_lane: D is no multiple of 16)
    S[0, 2, D - 2] = 10                              # last_lane only
    S[0, 3, 2] = S[0, 3, 18] = 10                    # tie, 16 apart
    S[0, 4, 5] = 550
    S[0, 4, 9] = 555                                 # margin = (uint16)(550 * 0.0099999905) = 5: gap_eq
    S[0, 5, 5] = 550
    S[0, 5, 9] = 556                                 # gap_eq1
    S[0, 6, 5] = 10
    S[0, 6, 4] = 65535                               # edge_cost; (int16) -1 + 1000 - 20 >= 1: not flat
    S[0, 7, :] = 65535                               # none
    c = WC.classify(S, D, 0, True, 0.99)["left"]["classes"]
    got = {n: np.nonzero(m[0])[0].tolist() for n, m in c.items()}
    assert got == {"first": [0], "last": [1], "last_lane": [1, 2], "tie": [3], "tie_far": [3], "gap_eq": [4], "gap_eq1": [5],
                   "flat": [], "edge_cost": [6], "none": [7]}
    S[0, 6, 6] = 12                                  # -1 + 12 - 20 < 1: the clamp
    c = WC.classify(S, D, 0, True, 0.99)["left"]
    assert np.nonzero(c["classes"]["flat"][0])[0].tolist() == [6]
    assert c["disp"][0, 6] == np.float32(5) + np.float32(-1 - 12) / np.float32(2)
