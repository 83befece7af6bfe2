"""The map stages behind the winner-take-all, branch by branch -- TEST INFRASTRUCTURE ONLY: planted inputs for the three LR checks
(csrc/sgm_sum_wta.hip), the classification and the fill passes (csrc/sgm_fill.hip), and a census that says which branch of the
contract every pixel takes.  A plain helper module, no fixtures; shared by tests/golden/make_golden_post_classes.py,
test_post_classes_cpu.py and test_gpu_post_classes.py.

The restatements the kernels are held to are the existing ones and nothing here says them again: the left check is the oracle's
sgmo_lrcheck, the right check its sgmo_lrcheck_right, the both-views check those two on copies of the raw maps, the classes
fill_holes_ref.classify, the passes fill_holes_ref._pass / fill.  The census below is the one second statement; the tests assert it
equal to them on every input (class 1 == back_inf | back_gt; class != 0 == inf | out_lo | out_hi | fail == where the LR output is
+INF).

census(ref, oth, thres, right): boolean masks per pixel of the reference view (sign - in the left view, + in the right one):
  inf         d == +INF
  out_lo/hi   the column (int)((double)((float)x -+ d) + 0.5) is < 0 / >= W
  trunc0      -1 < (double)((float)x -+ d) + 0.5 < 0: truncation gives column 0, a floor would give -1
  half        the float32 sum has fraction exactly .5
  f32_sum     the column differs from the one an exact (double) sum gives
  other_inf   the other view's value at the column is +INF: kept
  eq_thres    |d - o| == (double)thres: kept           ulp_over   (double)thres < |d - o| <= nextafter(thres): rejected
  pass / fail compared and kept / compared and rejected (eq_thres is a pass, ulp_over a fail)
  among fail, xb the column the other view's pixel points back at:
  back_lo/hi  xb outside the frame: class 2             back_inf   ref[xb] == +INF: class 1
  back_eq     ref[xb] == d: class 2                     back_gt / back_lt   ref[xb] > d: class 1 / ref[xb] < d: class 2

fill_census(disp, cls, R): per pass (1, 2, 3) masks per pixel -- of its targets k0 .. k8 (by number of candidates), hit_at_R (a
ray collects its value at step R exactly), miss_past_R (a ray's first finite value is at step R + 1, inside the frame), edge_stop (a
ray without a value ends at the frame edge before R), dup (the selected rank has an equal neighbour in the sorted list); of the
others copied_other_class (an INF pixel whose class is not the pass's) and valid_with_class (a finite pixel of class 1 or 2).

Planted inputs are batches of three DIFFERENT frames from a seed, so that a read across a row end or a frame edge changes the
result; values are quarter-pel but for the planted float32-sum and threshold pixels; a share of the disparities is negative (the
kernels take any finite float; out_hi and back_lo of the left view need one); about 15 % of either map is +INF."""
import ctypes as C
import functools

import numpy as np

import fill_holes_ref as F

INF = np.float32(np.inf)
F32, F64 = np.float32, np.float64
VIEWS = ("left", "right")
LR_BRANCHES = ("inf", "out_lo", "out_hi", "trunc0", "half", "f32_sum", "other_inf", "eq_thres", "ulp_over", "pass", "fail",
               "back_lo", "back_hi", "back_inf", "back_eq", "back_gt", "back_lt")
FILL_K = tuple(f"k{i}" for i in range(9))
FILL_MASKS = FILL_K + ("hit_at_R", "miss_past_R", "edge_stop", "dup", "copied_other_class", "valid_with_class")
FLOOR = 20                                   # pixels (targets) per branch: keeps a test from passing on one lucky pixel
B = 3

# ---- the device layer's geometry (csrc/sgm_device.h, sgmd_geom); test_post_classes_cpu.py compares it with the header's text ----

GEOM_FIELDS = ("W", "H", "D", "Dp", "DPL", "LPP", "HL", "dmin", "B", "row_begin", "row_end")


class Geom(C.Structure):
    _fields_ = [(n, C.c_int) for n in GEOM_FIELDS]


def geom(W, H, frames, row_begin=0, row_end=None):
    """the geometry of `frames` maps of W x H (the disparity range is of no concern to the map kernels: 16 cells, padded to 32)"""
    return Geom(W=W, H=H, D=16, Dp=32, DPL=2, LPP=16, HL=0, dmin=0, B=frames, row_begin=row_begin, row_end=H if row_end is None else row_end)


# ---- the restatements, per batch ------------------------------------------------------------------------------------------------

def lr_left(oracle, dl, dr, thres):
    return np.stack([oracle.lrcheck(dl[f], dr[f], thres) for f in range(dl.shape[0])])


def lr_right(oracle, dr, dl, thres):
    fn = oracle.lib.sgmo_lrcheck_right
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float], None
    out = np.array(dr, np.float32, copy=True, order="C")
    other = np.ascontiguousarray(dl, np.float32)
    h, w = out.shape[-2:]
    for f in range(out.shape[0]):
        fn(out[f].ctypes.data, other[f].ctypes.data, w, h, thres)
    return out


def lr_both(oracle, dl, dr, thres):
    """either check on the RAW maps"""
    return lr_left(oracle, dl, dr, thres), lr_right(oracle, dr, dl, thres)


def classes(ref, oth, thres, right):
    return np.stack([F.classify(ref[f], oth[f], thres, right=right) for f in range(ref.shape[0])])


def fill_passes(disp, cls, R):
    """[after pass 1, after pass 2, after pass 3] of a batch, each pass on the one before (fill_holes_ref._pass per frame)"""
    outs, m = [], np.array(disp, np.float32, copy=True)
    for p in (1, 2, 3):
        m = np.stack([F._pass(m[f], (m[f] == INF) & (True if p == 3 else cls[f] == p), R, p == 1) for f in range(m.shape[0])])
        outs.append(m)
    return outs


# ---- the census of the LR checks and the classes ---------------------------------------------------------------------------------

def column(x, sd):
    """the contract's column of x and the SIGNED disparity sd: (float32 sum, its double + 0.5, that truncated toward zero)"""
    s32 = np.asarray(x).astype(F32) + np.asarray(sd, F32)
    t = s32.astype(F64) + 0.5
    return s32, t, np.trunc(t).astype(np.int64)


def census(ref, oth, thres, right):
    ref, oth = np.asarray(ref, F32), np.asarray(oth, F32)
    W = ref.shape[-1]
    x = np.broadcast_to(np.arange(W), ref.shape)
    sgn = F32(1) if right else F32(-1)
    inf = ref == INF
    fin = ~inf
    d = np.where(fin, ref, F32(0))
    s32, t, col = column(x, sgn * d)
    exact = np.trunc(x.astype(F64) + F64(sgn) * d.astype(F64) + 0.5).astype(np.int64)
    out_lo, out_hi = fin & (col < 0), fin & (col >= W)
    inb = fin & (col >= 0) & (col < W)
    o = np.take_along_axis(oth, np.clip(col, 0, W - 1), axis=-1)
    other_inf = inb & (o == INF)
    cmp = inb & (o != INF)
    o0 = np.where(cmp, o, F32(0))
    diff = np.abs((d - o0).astype(F64))                      # the difference is a float32 one
    thr, up = F64(F32(thres)), F64(np.nextafter(F32(thres), INF))
    fail = cmp & (diff > thr)
    _, _, xb = column(col, -sgn * o0)
    back_in = fail & (xb >= 0) & (xb < W)
    r = np.take_along_axis(ref, np.clip(xb, 0, W - 1), axis=-1)
    return {"inf": inf, "out_lo": out_lo, "out_hi": out_hi, "trunc0": fin & (t > -1) & (t < 0), "half": fin & (s32 - np.floor(s32) == F32(0.5)),
            "f32_sum": fin & (col != exact), "other_inf": other_inf, "eq_thres": cmp & (diff == thr), "ulp_over": fail & (diff <= up),
            "pass": cmp & ~fail, "fail": fail, "back_lo": fail & (xb < 0), "back_hi": fail & (xb >= W), "back_inf": back_in & (r == INF),
            "back_eq": back_in & (r == d), "back_gt": back_in & (r != INF) & (r > d), "back_lt": back_in & (r < d)}


def counts(masks):
    return {n: int(m.sum()) for n, m in masks.items()}


# ---- planted LR inputs -----------------------------------------------------------------------------------------------------------

# name: (W, H, thres, seed, kind) -- kind "planted": random maps with every branch placed; "random": the degenerate shapes, random maps
# alone; "f32": k + 0.5 +- j * 0.0009 at columns past 2^15, where the float32 sum and the exact one part ways thousands of times
LR_INPUTS = {
    "96x24": (96, 24, 1.0, 0x9C01, "planted"),
    "257x5": (257, 5, 1.0, 0x9C02, "planted"),
    "96x24-t0.1": (96, 24, 0.1, 0x9C03, "planted"),
    "256x4": (256, 4, 1.0, 0x9C04, "planted"),
    "255x3": (255, 3, 1.0, 0x9C05, "planted"),
    "33x7": (33, 7, 1.0, 0x9C06, "planted"),
    "3x3": (3, 3, 1.0, 0x9C07, "random"),
    "1x1": (1, 1, 1.0, 0x9C08, "random"),
    "65535x2": (65535, 2, 1.0, 0x9C09, "f32"),
}
QUOTA_INPUTS = ("96x24", "257x5", "96x24-t0.1")         # the quota shapes, the second threshold included
TINY = (-(0.5 + 2.0 ** -24), 0.5 - 2.0 ** -25, -(1.5 + 2.0 ** -23), 1.5 - 2.0 ** -23)   # signed disparities a float32 sum rounds across .5


class LRInput:
    def __init__(self, name):
        self.name = name
        self.W, self.H, self.thres, self.seed, self.kind = LR_INPUTS[name]
        rng = np.random.default_rng(self.seed)
        make = {"planted": _planted_frame, "random": _random_frame, "f32": _f32_frame}[self.kind]
        frames = [make(rng, self.W, self.H, self.thres) for _ in range(B)]
        self.dl = np.stack([f[0] for f in frames])
        self.dr = np.stack([f[1] for f in frames])
        for a in (self.dl, self.dr):
            a.setflags(write=False)

    def view(self, right):
        """(reference view's raw map, the other view's)"""
        return (self.dr, self.dl) if right else (self.dl, self.dr)

    def census(self, right):
        return census(*self.view(right), self.thres, right)

    def counts(self):
        return {v: counts(self.census(v == "right")) for v in VIEWS}


@functools.lru_cache(maxsize=None)
def lr_input(name):
    return LRInput(name)


def _random_map(rng, W, H, lo, hi):
    m = (rng.integers(lo, hi, (H, W)) / F32(4)).astype(F32)
    m[rng.random((H, W)) < 0.15] = INF
    return m


def _random_frame(rng, W, H, thres):
    return _random_map(rng, W, H, -4, 12), _random_map(rng, W, H, -4, 12)


def _f32_frame(rng, W, H, thres):
    def one():
        k, j = rng.integers(-8, 64, (H, W)), rng.integers(-4, 5, (H, W))
        m = (k + 0.5 + j * 0.0009).astype(F32)
        m[rng.random((H, W)) < 0.15] = INF
        return m
    return one(), one()


class _Planter:
    """places pixels of one branch of one view into a pair of maps; a cell somebody placed or relies on is locked in its map"""

    def __init__(self, rng, dl, dr):
        self.rng, self.maps = rng, (dl, dr)
        self.locks = (np.zeros(dl.shape, bool), np.zeros(dl.shape, bool))
        self.H, self.W = dl.shape

    @staticmethod
    def col(x, sd):
        return int(np.trunc(F64(F32(x) + F32(sd)) + 0.5))

    def put(self, right, y, x, d, o=None, back=None):
        """ref[y][x] = d; with o the other view's value at the column d points at; with back ref at the column o points back at"""
        ref, oth = (self.maps[1], self.maps[0]) if right else self.maps
        lref, loth = (self.locks[1], self.locks[0]) if right else self.locks
        sgn = 1.0 if right else -1.0
        if lref[y, x]:
            return False
        c = xb = None
        if o is not None:
            c = self.col(x, sgn * d)
            if not 0 <= c < self.W or loth[y, c]:
                return False
            if back is not None:
                xb = self.col(c, -sgn * o)
                if not 0 <= xb < self.W or xb == x or lref[y, xb]:
                    return False
        ref[y, x], lref[y, x] = F32(d), True
        if c is not None:
            oth[y, c], loth[y, c] = F32(o), True
        if xb is not None:
            ref[y, xb], lref[y, xb] = F32(back), True
        return True

    def quarter(self, lo, hi):
        return float(self.rng.integers(lo, hi)) / 4.0

    def place(self, n, right, recipe, x_lo, x_hi):
        """n pixels by recipe(y, x, sgn) -> arguments of put, or None; columns x_lo <= x < x_hi"""
        done, tries = 0, 0
        while done < n and tries < 60 * n:
            tries += 1
            y, x = int(self.rng.integers(self.H)), int(self.rng.integers(x_lo, x_hi))
            args = recipe(y, x, 1.0 if right else -1.0)
            done += bool(args is not None and self.put(right, y, x, *args))
        return done


def _threshold_pair(p, T):
    """(d, o) with |(float)(d - o)| == T exactly, d a small quarter-pel value; None where float32 has none"""
    for k in p.rng.permutation(12):
        d = F32(k / 4.0)
        for o in (F32(d + T), F32(d - T)):
            if abs(F64(F32(d - o))) == F64(T):
                return float(d), float(o)
    return None


def _planted_frame(rng, W, H, thres):
    dl, dr = _random_map(rng, W, H, -8, 64), _random_map(rng, W, H, -8, 64)
    p = _Planter(rng, dl, dr)
    n = max(1, min(12, W * H // 100))
    T, T_up = F32(thres), np.nextafter(F32(thres), INF)
    q = p.quarter

    def failing(back):
        def recipe(y, x, sgn):
            d = q(0, 12)
            o = d + float(rng.choice((-1.0, 1.0))) * (1.5 + q(0, 8))
            return d, o, back(d)
        return recipe

    def back_outside(low):
        def recipe(y, x, sgn):
            d = q(0, 12)
            c = p.col(x, sgn * d)
            return d, (sgn * (c + 1.5 + q(0, 8)) if low else -sgn * ((W - c) - 0.5 + q(0, 8)))
        return recipe

    recipes = [
        (lambda y, x, sgn: (sgn * -(x + 1.5 + q(0, 8)),), 0, W),                                    # out_lo
        (lambda y, x, sgn: (sgn * ((W - x) - 0.5 + q(0, 8)),), 0, W),                               # out_hi
        (lambda y, x, sgn: (sgn * (-x - float(rng.choice((0.75, 1.0, 1.25)))),), 0, W),             # trunc0
        (lambda y, x, sgn: (sgn * TINY[int(rng.integers(4))],), 8, W - 4),                           # f32_sum
        (lambda y, x, sgn: _threshold_pair(p, T), 4, W - 4),                                         # eq_thres
        (lambda y, x, sgn: _threshold_pair(p, T_up), 4, W - 4),                                      # ulp_over
        (back_outside(True), 8, W - 8), (back_outside(False), 8, W - 8),                             # back_lo, back_hi
        (failing(lambda d: INF), 8, W - 8), (failing(lambda d: d), 8, W - 8),                        # back_inf, back_eq
        (failing(lambda d: d + q(1, 9)), 8, W - 8), (failing(lambda d: d - q(1, 9)), 8, W - 8),      # back_gt, back_lt
    ]
    for right in (False, True):
        for recipe, x_lo, x_hi in recipes:
            p.place(n, right, recipe, x_lo, x_hi)
    return dl, dr


# ---- the census of the fill passes -----------------------------------------------------------------------------------------------

def _rays(m, ty, tx):
    """[8][n] per ray of the targets (ty, tx) of frame m: the step of the first finite value inside the frame (0: none), that value,
    and the steps to the frame edge"""
    h, w = m.shape
    n = ty.size
    step, val, edge = np.zeros((8, n), np.int64), np.full((8, n), INF, F32), np.zeros((8, n), np.int64)
    far = np.full(n, max(h, w), np.int64)
    for k, (dx, dy) in enumerate(F.RAYS):
        ex = far if dx == 0 else (w - 1 - tx if dx > 0 else tx)
        ey = far if dy == 0 else (h - 1 - ty if dy > 0 else ty)
        edge[k] = np.minimum(ex, ey)
        for s in range(1, max(h, w)):
            act = np.flatnonzero((step[k] == 0) & (s <= edge[k]))
            if act.size == 0:
                break
            v = m[ty[act] + dy * s, tx[act] + dx * s]
            hit = v != INF
            step[k, act[hit]], val[k, act[hit]] = s, v[hit]
    return step, val, edge


def _census_pass(m, cls, R, p):
    """(masks, the map after the pass) of pass p on frame m"""
    holes = m == INF
    targets = holes & (True if p == 3 else cls == p)
    masks = {n: np.zeros(m.shape, bool) for n in FILL_MASKS}
    if cls is not None:
        masks["copied_other_class"] = holes & ~targets
        masks["valid_with_class"] = ~holes & (cls != 0)
    out = m.copy()
    ty, tx = np.nonzero(targets)
    if ty.size:
        step, val, edge = _rays(m, ty, tx)
        within = (step >= 1) & (step <= R)
        k = within.sum(axis=0)
        s = np.sort(np.where(within, val, INF), axis=0)
        pick = np.where(k >= 2, 1, 0) if p == 1 else k // 2
        at = np.arange(ty.size)
        sel = s[pick, at]
        dup = (sel != INF) & (((pick > 0) & (s[np.maximum(pick - 1, 0), at] == sel)) | ((pick < 7) & (s[np.minimum(pick + 1, 7), at] == sel)))
        for i in range(9):
            masks[f"k{i}"][ty, tx] = k == i
        masks["hit_at_R"][ty, tx] = (step == R).any(axis=0)
        masks["miss_past_R"][ty, tx] = (step == R + 1).any(axis=0)
        masks["edge_stop"][ty, tx] = ((step == 0) & (edge < R)).any(axis=0)
        masks["dup"][ty, tx] = dup
        out[ty, tx] = sel
    return masks, out


def fill_census(disp, cls, R):
    """{pass: masks [B][H][W]} and {pass: the batch after it}; cls None: pass 3 alone"""
    disp = np.asarray(disp, F32)
    masks, outs, m = {}, {}, disp
    for p in ((1, 2, 3) if cls is not None else (3,)):
        per = [_census_pass(m[f], None if cls is None else cls[f], R, p) for f in range(m.shape[0])]
        masks[p] = {n: np.stack([q[0][n] for q in per]) for n in FILL_MASKS}
        outs[p] = m = np.stack([q[1] for q in per])
    return masks, outs


# ---- planted fill inputs ---------------------------------------------------------------------------------------------------------

FILL_SHAPES = {"61x47": (61, 47), "17x5": (17, 5), "5x17": (5, 17), "3x3": (3, 3), "1x9": (1, 9), "9x1": (9, 1)}
FILL_VARIANTS = ("bands", "edges")
FILL_RS = (1, 2, 7, 64)                                  # 64 >= max(W, H) of every shape: only the frame edge ends a walk
FILL_QUOTA_SHAPES = ("61x47", "17x5")
FILL_INPUTS = [(s, v) for s in FILL_SHAPES for v in FILL_VARIANTS]
# pass 3 takes every INF pixel: none is copied for its class
FILL_EXCUSED = {1: (), 2: (), 3: ("copied_other_class",)}


class FillInput:
    """bands: every frame in three bands of 10 %, 50 % and 95 % +INF along its longer side, the order turned from frame to frame;
    edges: a frame all finite, then one whose only finite pixel is its first (the corner next to the frame before it in memory), then
    one all +INF"""

    def __init__(self, shape, variant):
        self.name, self.shape, self.variant = f"{shape}-{variant}", shape, variant
        self.W, self.H = FILL_SHAPES[shape]
        self.seed = 0xF100 + 16 * list(FILL_SHAPES).index(shape) + FILL_VARIANTS.index(variant)
        rng = np.random.default_rng(self.seed)
        W, H = self.W, self.H
        disp = (rng.integers(-8, 64, (B, H, W)) / F32(4)).astype(F32)
        if variant == "bands":
            along = np.arange(W)[None, :] * 3 // W if W >= H else np.arange(H)[:, None] * 3 // H
            for f in range(B):
                share = np.asarray((0.10, 0.50, 0.95))[(along + f) % 3]
                disp[f][rng.random((H, W)) < share] = INF
        else:
            corner = disp[1, 0, 0]
            disp[1:] = INF
            disp[1, 0, 0] = corner
        self.disp = disp
        self.cls = rng.integers(0, 3, (B, H, W)).astype(np.uint8)
        for a in (self.disp, self.cls):
            a.setflags(write=False)

    def counts(self, R):
        masks, _ = fill_census(self.disp, self.cls, R)
        return {str(p): counts(m) for p, m in masks.items()}


@functools.lru_cache(maxsize=None)
def fill_input(shape, variant):
    return FillInput(shape, variant)


# ---- refinement inputs at the line lengths of the slab logic ------------------------------------------------------------------------

# (W, H, B): one sample; lines of 2; W <= 32 (the first slab is the last); W a multiple of 32; 33 (a last slab of one sample); H of
# 1 and 2; B * H of 63, 64 and 65 rows for the waves of 64
REFINE_SHAPES = [(1, 1, 1), (2, 2, 1), (1, 65, 1), (65, 1, 3), (31, 65, 1), (32, 64, 1), (33, 2, 3), (63, 3, 3), (64, 63, 2), (65, 64, 1),
                 (96, 21, 3)]
REFINE_PARAMS = [(16.0, 1.5, 1), (64.0, 8.0, 3), (500.0, 0.3, 8)]


def refine_inputs(W, H, frames):
    """[(disp, conf, guide, the frames that are all +INF)]: the inputs of test_gpu_refine.py's crafted maps at any shape -- random
    disparities, half of them +INF but never the first or the last sample of a frame, random confidence of at least 1, a guide with a flat half; in frame 0
    one column (W > 2) and one row (H > 2) of confidence 0, so that other columns and rows keep their weight; the second frame of a
    batch all +INF, and for a single frame the all-+INF map as a second input of its own"""
    rng = np.random.default_rng(1000 * W + 10 * H + frames)
    disp = (rng.random((frames, H, W)) * 60).astype(F32)
    disp[rng.random((frames, H, W)) < 0.5] = INF
    for f in range(frames):                                  # two finite samples at least, where there are two: something to smooth
        for at, v in (((0, 0), 7.25), ((H - 1, W - 1), 21.5)):
            if disp[f][at] == INF:
                disp[f][at] = F32(v)
    conf = rng.integers(1, 65536, (frames, H, W)).astype(np.uint16)
    if W > 2:
        conf[0, :, W // 2] = 0
    if H > 2:
        conf[0, H // 2, :] = 0
    guide = rng.integers(0, 256, (frames, H, W)).astype(np.uint8)
    guide[0, :, W // 2:] //= 4
    if frames > 1:
        disp[1] = INF
        return [(disp, conf, guide, (1,))]
    return [(disp, conf, guide, ()), (np.full_like(disp, INF), conf, guide, (0,))]
