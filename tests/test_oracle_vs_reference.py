"""Our CPU restatement against the reference's own C on seeded random shapes and options -- every stage.  The expected values
are the sha256 digests of what the reference's own C (oracle/_ref, built by oracle/build_ref.sh) computed for these very cases,
stored in tests/golden/reference_stages.json by tests/golden/make_golden_reference_stages.py: nothing here needs the reference."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.pyoracle import DIRECTIONS, STAGE_NAMES, default_option, sha

# (w, h, d, seed) of the per-direction aggregation comparison
AGG_CASES = [(23, 17, 6, 1), (17, 23, 6, 2), (64, 9, 20, 3)]


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(GOLDEN, "reference_stages.json")) as f:
        return json.load(f)


def case_id(c):
    return f"{c[0]}x{c[1]}_d{c[2]}-{c[3]}_s{c[4]}"


def agg_id(c):
    return f"{c[0]}x{c[1]}_d{c[2]}_s{c[3]}"


def _same(a, want):
    """a holds the values of the reference's array `want` was made from (float32 maps: the same bit patterns)."""
    if list(a.shape) != want["shape"]:
        return False
    if str(a.dtype) != want["dtype"]:
        b = a.astype(want["dtype"])
        if not np.array_equal(b, a):
            return False
        a = b
    return sha(a) == want["sha256"]


def _cases():
    rng = np.random.RandomState(20261004)
    out = []
    for k in range(28):
        w = int(rng.randint(6, 120))
        h = int(rng.randint(6, 70))
        d = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 31, 32, 47, 64]))
        dmin = int(rng.choice([0, 0, 0, 1, 4, 9]))
        kw = dict(p1=int(rng.choice([0, 3, 10, 25, 90])), p2_init=int(rng.choice([0, 8, 150, 255, 1000])),
                  is_check_unique=bool(rng.rand() < 0.8), uniqueness_ratio=float(rng.choice([0.99, 0.95, 0.5, 1.0])),
                  is_check_lr=bool(rng.rand() < 0.8), lrcheck_thres=float(rng.choice([1.0, 0.0, 2.5])),
                  is_remove_speckles=bool(rng.rand() < 0.8), min_speckle_area=int(rng.choice([0, 1, 7, 50])))
        if dmin > 0 and kw["is_check_lr"] and not kw["is_check_unique"]:
            # the reference reads cost_local[65535 - dmin] here (right-view pixel with no in-image candidate,
            # SemiGlobalMatching.c:432-435) and segfaults: undefined behaviour, not a parity target
            kw["is_check_unique"] = True
        out.append((w, h, dmin, dmin + d, 1000 + k, kw))
    # a second draw with large disparity ranges (padded and unpadded volumes, every lane layout of the GPU kernels)
    rng2 = np.random.RandomState(20261005)
    for k in range(20):
        w = int(rng2.randint(6, 300))
        h = int(rng2.randint(6, 90))
        d = int(rng2.choice([65, 96, 100, 127, 128, 129, 160, 192, 200, 255, 256]))
        dmin = int(rng2.choice([0, 0, 2, 7]))
        kw = dict(p1=int(rng2.choice([0, 5, 10, 40])), p2_init=int(rng2.choice([0, 30, 150, 400])),
                  is_check_unique=True, uniqueness_ratio=float(rng2.choice([0.99, 0.9])),
                  is_check_lr=bool(rng2.rand() < 0.8), lrcheck_thres=float(rng2.choice([1.0, 0.5])),
                  is_remove_speckles=bool(rng2.rand() < 0.8), min_speckle_area=int(rng2.choice([5, 20, 50])))
        out.append((w, h, dmin, dmin + d, 2000 + k, kw))
    # hand-picked corners: negative penalties, the census no-op sizes, one-row / one-column images
    out += [(40, 20, 0, 16, 1, dict(p1=-7, p2_init=120)), (40, 20, 0, 16, 2, dict(p1=12, p2_init=-300)),
            (40, 20, 0, 16, 3, dict(p1=32767, p2_init=32767)), (5, 30, 0, 4, 4, {}), (30, 5, 0, 4, 5, {}),
            (1, 9, 0, 2, 6, {}), (9, 1, 0, 2, 7, {}), (2, 2, 0, 1, 8, {}), (3, 40, 0, 2, 9, {}),
            (64, 3, 0, 8, 10, dict(min_speckle_area=3))]
    return out


@pytest.mark.parametrize("case", _cases(), ids=case_id)
def test_all_stages_equal_reference(oracle, case):
    w, h, dmin, dmax, seed, kw = case
    want = _golden()["cases"][case_id(case)]
    assert want["options"] == kw                                # the fixture was made for this very case
    left, right = oracle.synth_pair(w, h, dmax - dmin, seed)
    assert sha(left) == want["sha256_inputs"]["left"] and sha(right) == want["sha256_inputs"]["right"]
    opt = default_option(dmax, dmin, **kw)
    got = oracle.run(left, right, opt)
    if not opt.is_check_lr:
        got["disp_r"][:] = 0
    for n in STAGE_NAMES:
        assert _same(got[n], want["stages"][n]), f"{case}: stage {n} differs"


def test_per_direction_aggregation_equal_reference(oracle):
    for (w, h, d, seed) in AGG_CASES:
        want = _golden()["aggregate_dir"][agg_id((w, h, d, seed))]
        left, right = oracle.synth_pair(w, h, d, seed)
        assert sha(left) == want["sha256_inputs"]["left"] and sha(right) == want["sha256_inputs"]["right"]
        opt = default_option(d)
        cost = oracle.run(left, right, opt)["cost"]
        assert _same(cost, want["cost"]), f"{(w, h)}: cost differs"
        for dx, dy in DIRECTIONS:
            S, _, _ = oracle.aggregate_dir(left, cost, opt.p1, opt.p2_init, dx, dy)
            assert _same(S, want["directions"][f"{dx},{dy}"]), f"{(w, h, dx, dy)}"
