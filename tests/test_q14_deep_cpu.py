"""A hundred matches without Reset on the CPU (tests/q14_deep.py): the oracle against what the compiled reference
made of the same sequences (tests/golden/q14_deep.json / .npz, make_golden_q14_deep.py), and the proof that those sequences reach
the regimes they are there for -- cost sums beyond 15 bits, wrapped sums, (int16) denominators below 1, best costs with bit 15
set.  Tolerance: 0, bit patterns.  The conditions below are properties of the fixed sequences, not tolerances: a changed
sequence has to be re-checked against them."""
import json
import os

import numpy as np
import pytest

import confidence_ref
import q14_deep as Q
from conftest import GOLDEN, load_npz
from oracle.pyoracle import sha

SHAPES = list(Q.FIXTURE_SHAPES)


@pytest.fixture(scope="module")
def fixture_json():
    with open(os.path.join(GOLDEN, "q14_deep.json")) as f:
        return json.load(f)["shapes"]


def seq(name):
    return Q.sequence(*Q.FIXTURE_SHAPES[name])


@pytest.mark.parametrize("name", SHAPES)
def test_oracle_reproduces_every_match_of_the_reference(fixture_json, name):
    fx, s = fixture_json[name], seq(name)
    assert (fx["w"], fx["h"], fx["dmin"], fx["dmax"]) == Q.FIXTURE_SHAPES[name] and fx["n"] == Q.N == s.n and fx["base"] == Q.BASE
    assert fx["min_speckle_area"] == s.option.min_speckle_area == Q.FIXTURE_SPECKLE_AREA
    for k, want in enumerate(fx["matches"]):
        assert sha(s.finals[k]) == want["sha256"], f"{name}: match {k} (no Reset since match 0) differs from the reference"
        assert int(np.isinf(s.finals[k]).sum()) == want["invalid"], f"{name}: match {k}"
    maps = load_npz(f"q14_deep_{name}.npz")
    assert sorted(maps) == sorted(f"final_{k}" for k in Q.FIXTURE_CHECKPOINTS[name])
    for k in Q.FIXTURE_CHECKPOINTS[name]:
        got, want = s.finals[k], maps[f"final_{k}"]
        assert sha(want) == fx["matches"][k]["sha256"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{name}: final map of match {k}"


@pytest.mark.parametrize("name", SHAPES)
def test_sequences_reach_the_regimes(name):
    s = seq(name)
    rows = s.rows
    assert max(r["share15"] for r in rows) >= 0.10, "no match with 10 % of the cells >= 32768"
    assert sum(r["wrapped"] for r in rows) >= 1, "no uint16 sum ever wrapped"
    assert sum(r["denom_lt1"] for r in rows) >= 1, "no interior pixel with an (int16) denominator < 1"
    if name == "40x12_dmin3_d40":
        assert max(r["m1_hi"] for r in rows) >= 1, "no pixel whose best cost is >= 32768"
    # the checkpoints are what they are said to be
    cp = Q.FIXTURE_CHECKPOINTS[name]
    assert s.checkpoints == cp
    assert rows[cp[0]]["s_max"] < 32768 <= rows[cp[0] + 1]["s_max"]
    assert rows[cp[1]]["share15"] >= 0.10
    assert rows[cp[2]]["wrapped"] > 0 and all(r["wrapped"] == 0 for r in rows[:cp[2]])
    assert s.ever_wrapped_share[cp[3]] >= 0.9 * s.ever_wrapped_share[-1] > 0
    assert cp[4] == Q.N - 1


def test_counters_on_crafted_costs():
    """regime() on a volume small enough to check by hand: [1][3][4], dmin 0."""
    S0 = np.array([[[10, 5, 9, 20], [40000, 33000, 40000, 50000], [7, 65535, 3, 65535]]], np.uint16)
    S1 = S0.copy()
    S1[0, 0, 1] = 2                                                   # fell: counts as wrapped
    r = Q.regime(S0, S1)
    assert r["wrapped"] == 1 and r["n_ffff"] == 2 and r["s_max"] == 65535 and abs(r["share15"] - 6 / 12) < 1e-12
    # pixel 1: best 33000 at index 1, neighbours 40000 = -25536 as int16: denominator (int16)(-51072 - 66000) = 14000 -> not < 1;
    # pixel 2: best 3 at index 2 between two 65535 = -1: denominator -2 - 6 = -8 < 1; pixel 0: 10 + 9 - 4 = 15
    assert r["denom_lt1"] == 1 and r["m1_hi"] == 1
    # right view of pixel x: S[x + k][k]; pixel 0: (10, 33000, 3, off the image) -> best at index 2, neighbours 33000 and 65535
    assert r["m1_hi_r"] == 1                                          # pixel 1: (40000, 65535, off, off)


@pytest.mark.parametrize("name", SHAPES)
def test_confidence_stays_within_u16_on_accumulated_costs(name):
    """(m2 - m1) * 65535 only just fits 32 bits: the confidence of tests/confidence_ref.py on the oracle's accumulated S, with the
    product taken in Python integers, is what the u32 arithmetic gives, and within [0, 65535]."""
    s = seq(name)
    dmin = Q.FIXTURE_SHAPES[name][2]
    for k in s.checkpoints:
        for right in (False, True):
            m1, m2, d1, conf = confidence_ref.confidence(s.stages[k]["aggr"], dmin, right)
            assert conf.dtype == np.uint16
            m1, m2 = m1.astype(object), m2.astype(object)
            assert (m2 >= m1).all() and (m2 <= 65535).all(), f"{name} match {k} right={right}"
            exact = np.where(m2 == 0, 0, (m2 - m1) * 65535 // np.where(m2 == 0, 1, m2))
            assert (exact >= 0).all() and (exact < 65536).all()
            assert ((m2 - m1) * 65535 < 2 ** 32).all()
            assert np.array_equal(exact.astype(np.uint16), conf), f"{name} match {k} right={right}"
