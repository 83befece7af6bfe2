"""Inputs of the temporal filter's kernel tests, shared by tests/test_temporal_cpu.py (the C stand-in against the numpy restatement,
and the class-coverage condition, both checkable without a GPU) and tests/test_gpu_temporal.py (the kernel against the same).

    SHAPES      (pixels, streams, steps[, misaligned])   PARAMS      (alpha, delta, n, k) as temporal_ref.Spec with min_conf
    inputs(shape, spec, seed)                            maps, conf, hv, hb of one kernel case
"""
import numpy as np

import temporal_ref as TR

MIN_CONF = 20000
# (pixels, streams, steps, misaligned): one pixel; three; pixel counts that are not multiples of four; one vector pass; several
# chunks; more than one pass of a capped grid on either path (one pixel per lane, four pixels per lane); maps offset by 4 bytes and
# the confidence by 2, which cannot be read 16 / 8 bytes at a time
SHAPES = [(1, 1, 1, False), (3, 1, 2, False), (777, 2, 3, False), (2310, 3, 8, False), (4096, 1, 8, False), (60000, 2, 4, False),
          (3000001, 1, 2, False), (2200004, 1, 1, False), (4096, 2, 3, True)]
PARAMS = [TR.Spec(0.4, 0.5, 3, 2, MIN_CONF), TR.Spec(1.0, 0.0, 0, 1, MIN_CONF), TR.Spec(0.0625, 1e30, 8, 8, MIN_CONF),
          TR.Spec(0.5, 0.125, 1, 1, MIN_CONF)]
# the decisions each parameter set admits (temporal_ref.CLASSES, "forgets" counting as one): without a hold window nothing is held
ADMITS = [("first", "smoothed", "replaced", "held", "invalid", "forgets"), ("first", "smoothed", "replaced", "invalid", "forgets"),
          ("first", "smoothed", "replaced", "held", "invalid", "forgets"), ("first", "smoothed", "replaced", "held", "invalid", "forgets")]


def shape_id(shape):
    return "%dx%dx%d%s" % (shape[0], shape[1], shape[2], "_misaligned" if shape[3] else "")


def inputs(shape, spec, seed=0):
    """maps f32 [streams][steps][pixels], conf u16 of that shape, hv f32 / hb u8 [streams][pixels].
    Base disparities in [0, 64) on a quarter-pixel grid; every step adds a change drawn from {0, +-2^-6, +-delta exactly,
    +-nextafter(delta), +-3}; a fifth of the entries is then planted as +INF, -INF or NaN.  The history: hv is the base value for
    half of the pixels (so that the first step's change IS x - hv, the gate hit exactly), a random value in [0, 64) for the rest,
    +INF for a fifth of all; hb random, an eighth of them 0xFF or 0x80 (the states from which one step holds with k = n = 8, or
    forgets)."""
    pixels, streams, steps = shape[:3]
    rng = np.random.RandomState(0x7E4D + 977 * seed + pixels % 65521 + 31 * streams + 7 * steps)
    delta = np.float32(spec.delta)
    up = np.nextafter(delta, np.float32(np.inf), dtype=np.float32)
    changes = np.array([0, 2.0 ** -6, -2.0 ** -6, delta, -delta, up, -up, 3, -3], np.float32)
    base = (rng.randint(0, 256, (streams, pixels)).astype(np.float32) / np.float32(4)).astype(np.float32)
    maps = np.empty((streams, steps, pixels), np.float32)
    x = base
    for t in range(steps):
        with np.errstate(all="ignore"):
            x = (x + changes[rng.randint(0, len(changes), (streams, pixels))]).astype(np.float32)
        maps[:, t] = x
    planted = rng.randint(0, 15, maps.shape)                                   # 0, 1, 2 of 15: a fifth
    maps[planted == 0] = np.inf
    maps[planted == 1] = -np.inf
    maps[planted == 2] = np.nan
    conf = rng.randint(0, 65536, maps.shape).astype(np.uint16)
    hv = np.where(rng.randint(0, 2, base.shape) == 0, base, (rng.randint(0, 256, base.shape) / 4.0)).astype(np.float32)
    hv[rng.randint(0, 5, base.shape) == 0] = np.inf
    hb = rng.randint(0, 256, base.shape).astype(np.uint8)
    special = rng.randint(0, 16, base.shape)
    hb[special == 0] = 0xFF
    hb[special == 1] = 0x80
    return maps, conf, hv, hb


def histogram(spec, maps, conf, hv, hb):
    """how often each decision of temporal_ref.CLASSES occurs, and "forgets": a finite hv that the call left not finite at some step"""
    streams, steps, pixels = maps.shape
    counts = dict.fromkeys(TR.CLASSES + ("forgets",), 0)
    hv, hb = hv.copy(), hb.copy()
    for t in range(steps):
        before = TR.finite_bits(hv.view(np.uint32))
        _, hv, hb, stats = TR.run(spec, maps[:, t:t + 1], None if conf is None else conf[:, t:t + 1], hv, hb)
        for c, name in enumerate(TR.CLASSES):
            counts[name] += int(stats[:, c].sum())
        counts["forgets"] += int((before & ~TR.finite_bits(hv.view(np.uint32))).sum())
    return counts


# ---- sequences of frames through the match ---------------------------------------------------------------------------------------

MATCH_SPEC = TR.Spec(0.4, 0.125, 3, 2)
PAIRS = ("t24x16_d8", "t70x33_d16", "t20x31_d8_tall", "t40x24_d16_dmin3", "t33x33_d12_square", "t64x20_d40", "cone")
FRAMES = 6
BLANK = 3                       # the frame whose right image is the constant 128: almost entirely invalid


def frames_of(left, right, first=0, count=FRAMES, blank=BLANK):
    """frame k of a sequence: the pair plus np.random.RandomState(0x7E4D00 + k).randint(-3, 4) noise on left, then on right,
    clipped to u8; frame `blank`'s right image is replaced by the constant 128"""
    out = []
    for k in range(first, first + count):
        rs = np.random.RandomState(0x7E4D00 + k)
        l = np.clip(left.astype(np.int32) + rs.randint(-3, 4, left.shape), 0, 255).astype(np.uint8)
        r = np.clip(right.astype(np.int32) + rs.randint(-3, 4, right.shape), 0, 255).astype(np.uint8)
        if k == blank:
            r = np.full_like(r, 128)
        out.append((l, r))
    return out


def filtered(spec, finals, confs=None, hv=None, hb=None):
    """the maps of consecutive frames of ONE stream through the reference filter, one step at a time:
    [(out, hv, hb, counts[5])] per frame, each [H][W]"""
    shape = finals[0].shape
    if hv is None:
        hv, hb = TR.empty(1, finals[0].size)
    rows = []
    for k, m in enumerate(finals):
        conf = None if confs is None else confs[k].reshape(1, 1, -1)
        out, hv, hb, stats = TR.run(spec, m.reshape(1, 1, -1), conf, hv, hb)
        rows.append((out.reshape(shape), hv.reshape(shape).copy(), hb.reshape(shape).copy(), stats[0].copy()))
    return rows
