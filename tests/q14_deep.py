"""Long runs of SGM_Match without SGM_Reset: the sequence of frames, the counters that say which regime the
uint16 cost sums S are in, and the oracle's side of the comparison -- shared by tests/golden/make_golden_q14_deep.py,
test_q14_deep_cpu.py and test_gpu_q14_deep.py.  A plain helper module, no fixtures.

One match adds at most 8 x 255 (+ the second visits of the anomalous lines) to a cell, so S passes 2^15 after some 25 matches --
from where the reference's (int16) casts of S[best -+ 1] and of the parabola's denominator stop being the identity -- and passes
2^16, where the uint16 sums wrap, after some 50.

Frame k of a (w, h, dmin, dmax, base) sequence is synth_pair(w, h, dmax - dmin, base + k); for odd k the right image is replaced
by the LEFT image of synth_pair(w, h, dmax - dmin, 0x77 + k), an unrelated picture: costs stay high and the matches varied."""
import functools

import numpy as np

import confidence_ref

N = 100                     # matches per sequence unless a shape says otherwise
BASE = 0x5EED4000

# The two sequences tests/golden/q14_deep.json pins with the compiled reference: name -> (w, h, dmin, dmax); N matches from BASE,
# default options with min_speckle_area = 8.
FIXTURE_SHAPES = {"48x20_d16": (48, 20, 0, 16), "40x12_dmin3_d40": (40, 12, 3, 43)}
# Matches whose full final maps the fixture stores = what pick_checkpoints() gives for these sequences (test_q14_deep_cpu.py
# checks that against the oracle's S): the last match before any cell reaches 32768, the first with the largest share of cells
# there, the first with a wrapped cell, the first by which most of the wrapping cells have wrapped, the last match.
FIXTURE_CHECKPOINTS = {"48x20_d16": (23, 34, 48, 61, 99), "40x12_dmin3_d40": (23, 36, 48, 62, 99)}
FIXTURE_SPECKLE_AREA = 8


def frame(synth, w, h, dmin, dmax, base, k):
    """Frame k of the sequence; synth = the oracle's (or the library's) seeded generator synth_pair(w, h, d, seed)."""
    d = dmax - dmin
    left, right = synth(w, h, d, base + k)
    if k & 1:
        right = synth(w, h, d, 0x77 + k)[0]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def _view_counters(S, dmin, right):
    """(pixels with an interior best disparity and an (int16) parabola denominator < 1, pixels with m1 >= 32768) of one view"""
    m1, _, d1, _ = confidence_ref.confidence(S, dmin, right)
    c = confidence_ref.view_costs(S, dmin, right).astype(np.uint16)
    D = c.shape[2]
    interior = (d1 > 0) & (d1 < D - 1)
    kk = np.clip(d1, 1, max(D - 2, 1))[..., None]
    c1 = np.take_along_axis(c, kk - 1, axis=2)[..., 0].view(np.int16).astype(np.int64)
    c2 = np.take_along_axis(c, np.minimum(kk + 1, D - 1), axis=2)[..., 0].view(np.int16).astype(np.int64)
    denom = (c1 + c2 - 2 * m1.astype(np.int64)).astype(np.int16)
    return int((interior & (denom < 1)).sum()), int(((m1 >= 32768) & (d1 >= 0)).sum())


def regime(S_prev, S, dmin=0):
    """Counters of one match's accumulated costs S (u16 [H][W][D]); S_prev = the match before (None for the first).
      share15   share of cells >= 32768
      wrapped   cells that fell since the previous match: a uint16 sum wrapped (a match only ever adds)
      denom_lt1 left-view pixels with an interior best disparity whose (int16) parabola denominator is < 1, so that the clamp to 1
                acts (without the casts it cannot be: S[best-1] > m1 and S[best+1] >= m1 for the first minimum)
      m1_hi     left-view pixels whose smallest cost is >= 32768 (keys with bit 31 set)
      denom_lt1_r, m1_hi_r   the same two of the right view (cost of pixel x at index k: S[y][x + dmin + k][k])
      s_max, n_ffff   largest cell, cells equal to the "off the image" value 65535"""
    S = np.asarray(S)
    dl, ml = _view_counters(S, dmin, False)
    dr, mr = _view_counters(S, dmin, True)
    return {"share15": float((S >= 32768).mean()),
            "wrapped": 0 if S_prev is None else int((S < S_prev).sum()),
            "denom_lt1": dl, "m1_hi": ml, "denom_lt1_r": dr, "m1_hi_r": mr,
            "s_max": int(S.max()), "n_ffff": int((S == 65535).sum())}


def pick_checkpoints(rows, ever_wrapped_share):
    """The matches worth a full comparison, from the per-match counters `rows` and the running share of cells that have wrapped at
    least once: the last match before any cell reaches 32768, the first with the largest share of cells >= 32768 (the 15-bit
    regime), the first with a wrapped cell, the first by which 90 % of the cells that wrap at all have done so, the last match.
    Entries a sequence never reaches are left out, duplicates merged."""
    n = len(rows)
    picks = {n - 1}
    high = [k for k in range(n) if rows[k]["s_max"] >= 32768]
    if high:
        if high[0] > 0:
            picks.add(high[0] - 1)
        top = max(r["share15"] for r in rows)
        picks.add(next(k for k in range(n) if rows[k]["share15"] == top))
    if ever_wrapped_share[-1] > 0:
        picks.add(next(k for k in range(n) if rows[k]["wrapped"] > 0))
        picks.add(next(k for k in range(n) if ever_wrapped_share[k] >= 0.9 * ever_wrapped_share[-1]))
    return tuple(sorted(picks))


class Sequence:
    """What the oracle makes of one sequence: finals[k] (float32 map of match k), rows[k] (regime counters), checkpoints and, at
    those (every match with keep_S), the stages aggr / disp_l / disp_r / after_lr."""
    STAGES = ("aggr", "disp_l", "disp_r", "after_lr")

    def __init__(self, w, h, dmin, dmax, n=N, base=BASE, right_view=False, honor=False, window=(5, 5), keep_S=False, **opt_kw):
        from oracle.pyoracle import Oracle, default_option
        opt_kw.setdefault("min_speckle_area", FIXTURE_SPECKLE_AREA)
        self.shape, self.n, self.base = (w, h, dmin, dmax), n, base
        self.option = default_option(dmax, dmin, **opt_kw)
        orc = Oracle()                                           # a context of its own: S belongs to this sequence alone
        orc.set_honor_num_paths(honor)
        assert orc.set_census_window(*window)
        orc.set_reference_view(right_view)
        assert orc.reset(w, h, self.option)
        self.frames = [frame(orc.synth_pair, w, h, dmin, dmax, base, k) for k in range(n)]
        self.finals, self.rows, all_stages = [], [], []
        prev, ever, self.ever_wrapped_share = None, None, []
        for k, (l, r) in enumerate(self.frames):
            out = orc.match(l, r)
            assert out is not None
            self.finals.append(out)
            st = {name: orc.stage(name) for name in self.STAGES}
            S = st["aggr"]
            self.rows.append(regime(prev, S, dmin))
            ever = np.zeros(S.shape, bool) if prev is None else (ever | (S < prev))
            self.ever_wrapped_share.append(float(ever.mean()))
            prev = S
            all_stages.append(st)
        self.checkpoints = pick_checkpoints(self.rows, self.ever_wrapped_share)
        self.stages = {k: all_stages[k] for k in (range(n) if keep_S else self.checkpoints)}
        # sequence() shares one object between tests: nobody gets to write into the expected values
        for a in [x for f in self.frames for x in f] + self.finals + [x for st in self.stages.values() for x in st.values()]:
            a.setflags(write=False)

    def summary(self):
        r = self.rows
        first = lambda f: next((k for k in range(self.n) if f(r[k])), None)       # noqa: E731
        return {"first_15bit": first(lambda x: x["s_max"] >= 32768), "first_wrap": first(lambda x: x["wrapped"] > 0),
                "max_share15": max(x["share15"] for x in r), "ever_wrapped": self.ever_wrapped_share[-1],
                "wrapped_cells": sum(x["wrapped"] for x in r), "denom_lt1": sum(x["denom_lt1"] for x in r),
                "first_denom_lt1": first(lambda x: x["denom_lt1"] > 0), "m1_hi": max(x["m1_hi"] for x in r),
                "denom_lt1_r": sum(x["denom_lt1_r"] for x in r), "m1_hi_r": max(x["m1_hi_r"] for x in r),
                "n_ffff": sum(x["n_ffff"] for x in r), "checkpoints": self.checkpoints}


@functools.lru_cache(maxsize=None)
def sequence(w, h, dmin, dmax, n=N, base=BASE, right_view=False, honor=False, window=(5, 5), keep_S=False, opt=()):
    """Sequence(...) computed once per process and shared by the tests that need it (its arrays are write-protected; a few MB at
    the sizes used, the largest the keep_S ones with every match's stages); opt = sorted option overrides as a tuple of
    (name, value)."""
    return Sequence(w, h, dmin, dmax, n, base, right_view, honor, window, keep_S, **dict(opt))
