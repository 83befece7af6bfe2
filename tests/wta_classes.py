"""The winner-take-all's decisions, counted: which branch of the reference's ComputeDisparity (SemiGlobalMatching.c:374-443) every
pixel of a frame takes, in numpy, from the summed costs S alone -- and seeded stereo pairs whose true disparity is planted so
that the branches seeded noise hardly ever reaches are taken by hundreds of pixels.  A plain helper module, no fixtures; shared by
tests/golden/make_golden_wta_classes.py, test_wta_classes_cpu.py and test_gpu_wta_classes.py.

Costs of a pixel, as include/sgm_mi355x.h documents them: left view S[y][x][k], right view S[y][x + dmin + k][k] and 65535 where
that column is off the image (k = d - dmin).  int64 / float32 are used where the reference's C uses int / float.

Classes of a pixel (m1 = smallest cost, d1 = first index reaching it, m2 = smallest cost at any other index, c1 / c2 = the (int16)
costs at d1 -+ 1, margin = (uint16)(m1 * (1 - uniqueness_ratio))):
  first      d1 == 0                                 last       d1 == D - 1
  last_lane  d1 == D - 1, or D - 2 as well where D is no multiple of 16 (the top slots of the last 16-lane group in use)
  tie        m1 is reached more than once            tie_far    ... at indices 16 or more apart
  gap_eq     m2 - m1 == margin, m2 > m1              gap_eq1    m2 - m1 == margin + 1
  flat       0 < d1 < D - 1, not rejected by the uniqueness test, (int16)(c1 + c2 - 2 m1) < 1: the clamp of the denominator to 1
  edge_cost  0 < d1 < D - 1 and the cost at d1 - 1 or d1 + 1 is 65535 (the cast makes it -1)
  none       no candidate: every cost is 65535"""
import functools

import numpy as np

import confidence_ref

INF = np.float32(np.inf)
CLASSES = ("first", "last", "last_lane", "tie", "tie_far", "gap_eq", "gap_eq1", "flat", "edge_cost", "none")
VIEWS = ("left", "right")


def quantities(S, D, dmin, ratio, right):
    """What the finish decides on, per pixel of one view: a dict of [H][W] int64 arrays (and the view's costs `c`)."""
    c = confidence_ref.view_costs(np.asarray(S)[..., :D], dmin, right).astype(np.int64)
    m1 = c.min(axis=2)
    hit = c == m1[..., None]
    d1 = np.argmax(hit, axis=2).astype(np.int64)
    d_last = (D - 1 - np.argmax(hit[..., ::-1], axis=2)).astype(np.int64)
    nobody = m1 >= 65535                                              # the reference's strict '>' from 65535 never fires
    d1[nobody] = -1
    others = c.copy()
    yy, xx = np.nonzero(~nobody)
    others[yy, xx, d1[yy, xx]] = 65536
    m2 = np.minimum(others.min(axis=2), 65535)
    margin = (m1.astype(np.float32) * (np.float32(1) - np.float32(ratio))).astype(np.uint16).astype(np.int64)
    kk = np.clip(d1, 1, max(D - 2, 1))[..., None]
    raw1 = np.take_along_axis(c, np.minimum(kk - 1, D - 1), axis=2)[..., 0]
    raw2 = np.take_along_axis(c, np.minimum(kk + 1, D - 1), axis=2)[..., 0]
    c1 = raw1.astype(np.uint16).view(np.int16).astype(np.int64)      # 65535 -> -1
    c2 = raw2.astype(np.uint16).view(np.int16).astype(np.int64)
    denom = (c1 + c2 - 2 * m1).astype(np.int16).astype(np.int64)
    return {"c": c, "m1": m1, "m2": m2, "d1": d1, "d_last": d_last, "n_min": hit.sum(axis=2), "margin": margin,
            "raw1": raw1, "raw2": raw2, "c1": c1, "c2": c2, "denom": denom}


def classes_of(q, D, unique):
    d1, m1, m2 = q["d1"], q["m1"], q["m2"]
    has = d1 >= 0
    interior = (d1 > 0) & (d1 < D - 1)
    kept = (m2 - m1 > q["margin"]) if unique else np.ones(d1.shape, bool)
    tie = has & (q["n_min"] > 1)
    return {"first": d1 == 0, "last": d1 == D - 1,
            "last_lane": (d1 == D - 1) | ((d1 == D - 2) & (D % 16 != 0) & (D >= 2)),
            "tie": tie, "tie_far": tie & (q["d_last"] - d1 >= 16),
            "gap_eq": has & (m2 > m1) & (m2 - m1 == q["margin"]), "gap_eq1": has & (m2 - m1 == q["margin"] + 1),
            "flat": interior & kept & (q["denom"] < 1),
            "edge_cost": interior & ((q["raw1"] == 65535) | (q["raw2"] == 65535)),
            "none": ~has}


def finish(q, D, dmin, unique):
    """The reference's finish (.c:412-440) on the quantities above: uniqueness, the border rule, the sub-pixel parabola with
    its (int16) casts and the clamp of the denominator; float32 as the C."""
    d1 = q["d1"]
    ok = d1 >= 0
    if unique:
        ok &= q["m2"] - q["m1"] > q["margin"]
    ok &= (d1 != 0) & (d1 != D - 1)
    denom = np.maximum(q["denom"], 1)
    val = (d1 + dmin).astype(np.float32) + (q["c1"] - q["c2"]).astype(np.float32) / (denom.astype(np.float32) * np.float32(2.0))
    return np.where(ok, val, INF).astype(np.float32)


def classify(S, D, dmin, unique=True, ratio=0.99):
    """{"left" / "right": {"classes": {name: bool [H][W]}, "disp": the restated finish's map}}"""
    out = {}
    for view in VIEWS:
        q = quantities(S, D, dmin, ratio, view == "right")
        out[view] = {"classes": classes_of(q, D, unique), "disp": finish(q, D, dmin, unique)}
    return out


def counts(S, D, dmin, unique=True, ratio=0.99):
    r = classify(S, D, dmin, unique, ratio)
    return {v: {n: int(m.sum()) for n, m in r[v]["classes"].items()} for v in VIEWS}


def floor(w, h):
    """The quota of a planted class: 50 pixels or 1 % of the frame, whichever is larger."""
    return max(50, -(-w * h // 100))


# --------------------------------------------------------------------------------------------------------------- planted inputs

def band_list(D):
    """The planted disparity indices k = d - dmin: both ends of the range, one beyond it, both sides of a 16-lane boundary, the
    middle, and for D > 64 both sides of every 64-index boundary inside it."""
    ks = [D - 1, 0, D - 2, 1, D, 15, 16, D // 2]
    if D > 64:
        ks = [D - 1, D - 2] + [k for k in (63, 64, 127, 128, 255, 256) if k < D] + ks[1:]
    seen, out = set(), []
    for k in ks:
        if k not in seen and k >= 0:
            seen.add(k)
            out.append(k)
    return out


def band_indices(D, n, part=0):
    """Bands of input `part`: the list in chunks of n -- what one frame cannot hold in 3-row bands goes to the next input."""
    return band_list(D)[part * n:(part + 1) * n]


def planted_pair(synth, w, h, dmin, D, seed, ks, flat=False):
    """Left: box-filtered LCG noise (synth_pair's left image).  Right: the left shifted by dmin + ks[b] in row band b, no
    jitter; columns whose source is off the image come from a second noise picture.  flat: a constant-grey patch (a third of the
    band wide, 12 columns at least) in every band, in the left image before the shift."""
    left = synth(w, h, max(D, 1), seed)[0].copy()
    fill = synth(w, h, max(D, 1), (seed * 2654435761 + 1) & 0xFFFFFFFF)[0]
    rows = np.array_split(np.arange(h), len(ks))
    assert all(len(r) >= 3 for r in rows), "bands are at least 3 rows tall"
    right = fill.copy()
    for b, (k, r) in enumerate(zip(ks, rows)):
        d = dmin + k
        if flat:
            fw = max(12, w // 3)
            x0 = min(max(d, 0) + 4 + 5 * b, max(w - fw - 2, 0))
            left[r[0]:r[-1] + 1, x0:x0 + fw] = 96 + 16 * (b % 4)
        if d < w:
            right[r[0]:r[-1] + 1, :w - d] = left[r[0]:r[-1] + 1, d:]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


# name of a shape -> (w, h, dmin, dmax); the padded disparity stride of the device kernels in the comment
SHAPES = {"64x16_d16": (64, 16, 0, 16),            # 32
          "150x27_d3-93": (150, 27, 3, 93),        # 128, dmin > 0, D = 90: padding cells, no multiple of 16
          "300x24_d128": (300, 24, 0, 128),        # 128
          "260x24_d192": (260, 24, 0, 192),        # 192
          "200x24_d256": (200, 24, 0, 256),        # 256, W < D
          "90x24_d512": (90, 24, 0, 512),          # 512: the separate sum / right-view kernels, W < D
          "140x24_d100": (140, 24, 0, 100),        # 128, padding cells
          "40x45_d8": (40, 45, 0, 8),              # 32, W < H
          # beyond the issue's eight.  Stride 64, which none of them selects; dmin > 0 at every stride (the right view's `none`
          # pixels are its last dmin columns); a full stride of 32 wide enough for four row segments of the fused kernel; index
          # D - 1 exists for a pixel only where W > dmin + D - 1: wide, low frames for the two widest layouts
          "96x24_d4-52": (96, 24, 4, 52),          # 64
          "288x16_d4-36": (288, 16, 4, 36),        # 32, D = 32
          "260x24_d3-195": (260, 24, 3, 195),      # 192
          "300x12_d5-261": (300, 12, 5, 261),      # 256
          "560x6_d9-521": (560, 6, 9, 521)}        # 512
ISSUE_SHAPES = tuple(SHAPES)[:8]

# name of a variant -> (bands per 24 rows, part of the band list, flat patches, option overrides)
# bands / bands2: the list above in 3-row bands, first and second chunk; p0: P1 = P2 = 0 (S = visits x Hamming cost: dense ties),
# no uniqueness test, taller bands with flat patches (p0u: the same with the uniqueness test on); top: the whole frame at index D - 1, the best a pixel can do being the last
# slot of the layout; noise: synth_pair as it is (costs in the hundreds, where the uniqueness margin is not 0: gap_eq)
VARIANTS = {"bands": (8, 0, False, {}),
            "bands2": (8, 1, False, {}),
            "p0": (4, 0, True, dict(p1=0, p2_init=0, is_check_unique=False)),
            "p0u": (4, 0, True, dict(p1=0, p2_init=0)),
            "top": (0, 0, False, {}),
            "noise": (None, 0, False, {})}
TOP_SHAPES = ("288x16_d4-36", "40x45_d8", "96x24_d4-52", "150x27_d3-93", "140x24_d100", "260x24_d192", "260x24_d3-195",
              "300x12_d5-261", "560x6_d9-521")
NOISE_SHAPES = ("64x16_d16", "40x45_d8", "288x16_d4-36", "96x24_d4-52", "90x24_d512", "560x6_d9-521")
P0U_SHAPES = ("96x24_d4-52",)
SPECKLE_AREA = 8


def n_bands(h, per24):
    return max(1, min(h * per24 // 24, h // 3))


def variants_of(shape):
    w, h, dmin, dmax = SHAPES[shape]
    out = ["bands"]
    if shape in ISSUE_SHAPES:                      # the low extra frames hold too few bands: they are there for the top index
        if len(band_list(dmax - dmin)) > n_bands(h, 8):
            out.append("bands2")
        out.append("p0")
    if shape in P0U_SHAPES:
        out.append("p0u")
    if shape in TOP_SHAPES:
        out.append("top")
    if shape in NOISE_SHAPES:
        out.append("noise")
    return out


class Planted:
    """One planted input: the pair, the options, and what the oracle makes of it (every stage, write-protected)."""

    def __init__(self, shape, variant, seed):
        from oracle.pyoracle import Oracle, default_option
        self.name, self.shape_name, self.variant, self.seed = f"{shape}-{variant}", shape, variant, seed
        w, h, dmin, dmax = self.shape = SHAPES[shape]
        per24, part, flat, kw = VARIANTS[variant]
        self.D = D = dmax - dmin
        self.option_kw = dict(min_speckle_area=SPECKLE_AREA, **kw)
        self.option = default_option(dmax, dmin, **self.option_kw)
        orc = Oracle()
        if per24 is None:
            self.ks = []
            self.left, self.right = orc.synth_pair(w, h, D, seed)
        else:
            self.ks = band_indices(D, n_bands(h, per24), part)
            self.left, self.right = planted_pair(orc.synth_pair, w, h, dmin, D, seed, self.ks, flat)
        self.stages = orc.run(self.left, self.right, self.option)
        for a in [self.left, self.right] + list(self.stages.values()):
            a.setflags(write=False)

    @property
    def unique(self):
        return bool(self.option.is_check_unique)

    def classify(self, S=None):
        return classify(self.stages["aggr"] if S is None else S, self.D, self.shape[2], self.unique, self.option.uniqueness_ratio)

    def counts(self, S=None):
        return counts(self.stages["aggr"] if S is None else S, self.D, self.shape[2], self.unique, self.option.uniqueness_ratio)


# the planted inputs: (shape, variant, seed); seeds chosen on the CPU so that the oracle alone meets the quotas of
# tests/golden/wta_classes.json
SEEDS = {("288x16_d4-36", "noise"): 0x7B69, ("96x24_d4-52", "noise"): 0x7B00}      # searched: tie_far / gap_eq above the floor
INPUTS = [(s, v, SEEDS.get((s, v), 0x7A00 + 16 * i + list(VARIANTS).index(v))) for i, s in enumerate(SHAPES) for v in variants_of(s)]


@functools.lru_cache(maxsize=None)
def planted(shape, variant, seed):
    """Planted(...) computed once per process, shared (and left unchanged) by the tests that need it."""
    return Planted(shape, variant, seed)


# ----------------------------------------------------------------------------------------------- matches without Reset (Q14)
# One match cannot take the clamp in the LEFT view: d1 is the first minimum, so S[d1 - 1] > m1 and the denominator is >= 1 -- until
# cells pass 32768 and the (int16) casts bite.  tests/q14_deep.py's sequences get S there; name -> (w, h, dmin, dmax, matches,
# option overrides): the S after the LAST match is the planted one (the match of the sequence with the most such pixels).
Q14_INPUTS = {"q14-48x20_d16": (48, 20, 0, 16, 59, ()),
              "q14-96x24_d48-interior": (96, 24, 0, 48, 60, (("p1", 32767), ("p2_init", 32767)))}
Q14_STAGES = ("aggr", "disp_l", "disp_r", "after_lr")


class Q14Planted:
    """q14_deep.Sequence run to its last match; stages = the oracle's aggr / disp_l / disp_r / after_lr / final after it."""

    def __init__(self, name):
        import q14_deep as Q
        w, h, dmin, dmax, n, opt = Q14_INPUTS[name]
        self.name, self.shape, self.D, self.n = name, (w, h, dmin, dmax), dmax - dmin, n
        self.seq = Q.sequence(w, h, dmin, dmax, n=n, opt=tuple(sorted(opt)))
        self.option, self.option_kw = self.seq.option, dict(opt, min_speckle_area=Q.FIXTURE_SPECKLE_AREA)
        self.frames, self.finals = self.seq.frames, self.seq.finals
        self.stages = dict(self.seq.stages[n - 1], final=self.seq.finals[n - 1])
        self.unique = True

    def counts(self, S=None):
        return counts(self.stages["aggr"] if S is None else S, self.D, self.shape[2], True, self.option.uniqueness_ratio)

    def classify(self, S=None):
        return classify(self.stages["aggr"] if S is None else S, self.D, self.shape[2], True, self.option.uniqueness_ratio)


@functools.lru_cache(maxsize=None)
def q14_planted(name):
    return Q14Planted(name)
