"""The temporal filter of include/sgm_mi355x.h (sgm_temporal_spec), restated in numpy: the reference the device and the C stand-in
(tests/stub_temporal.c) are compared with bit for bit.

    Spec(alpha, delta, n, k, min_conf)          the parameters the arithmetic looks at
    empty(streams, pixels)                      (hv, hb) of a history that has seen nothing: +INF / 0
    step(spec, hv, hb, x, conf)                 ONE step on arrays of pixels -> (out, hv', hb', cls)
    run(spec, maps, conf, hv, hb)               maps f32 [streams][steps][pixels] -> (out, hv', hb', stats u32 [streams * steps][5])

All arithmetic is float32, every operation rounded on its own (numpy rounds each array operation), subnormals kept.  "Finite" is
decided on the bit pattern; values that do not count never enter the arithmetic, and outputs are assembled from bit patterns so
that a NaN of the caller's comes through untouched where the contract passes a value on.
"""
import collections

import numpy as np

Spec = collections.namedtuple("Spec", "alpha delta n k min_conf", defaults=(0,))
CLASSES = ("first", "smoothed", "replaced", "held", "invalid")
INF_BITS = np.uint32(0x7F800000)


def finite_bits(u):
    return (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def empty(streams, pixels):
    return np.full((streams, pixels), np.inf, np.float32), np.zeros((streams, pixels), np.uint8)


def _popcount8(v):
    v = v.astype(np.uint8)
    return sum(((v >> i) & 1).astype(np.int32) for i in range(8))


def step(spec, hv, hb, x, conf=None):
    """One step (include/sgm_mi355x.h, "One step") on flat arrays: hv, x float32; hb uint8; conf uint16 or None."""
    a = np.float32(spec.alpha)
    b = np.float32(1.0) - a
    delta = np.float32(spec.delta)
    xb, hvb = x.view(np.uint32), hv.view(np.uint32)
    valid = finite_bits(xb)
    if conf is not None and spec.min_conf > 0:
        valid &= conf >= spec.min_conf
    hfin = finite_bits(hvb)
    cnt = _popcount8(hb & np.uint8((1 << spec.n) - 1))
    xs = np.where(valid, x, np.float32(0)).astype(np.float32)
    hs = np.where(hfin, hv, np.float32(0)).astype(np.float32)
    with np.errstate(all="ignore"):
        near = np.abs(xs - hs) <= delta
        smooth = (a * xs + b * hs).astype(np.float32)
    hold = ~valid & hfin & (cnt >= spec.k) if spec.n > 0 else np.zeros(x.shape, bool)
    cls = np.where(valid, np.where(hfin, np.where(near, 1, 2), 0), np.where(hold, 3, 4)).astype(np.uint8)
    out = np.select([cls == 1, cls == 3, cls == 4], [smooth.view(np.uint32), hvb, INF_BITS], xb).astype(np.uint32)
    hb2 = (((hb.astype(np.uint32) << 1) | valid) & 0xFF).astype(np.uint8)
    hv2 = np.where(finite_bits(out), out, np.where(hb2 == 0, INF_BITS, hvb)).astype(np.uint32)
    return out.view(np.float32), hv2.view(np.float32), hb2, cls


def run(spec, maps, conf, hv, hb):
    """maps float32 [streams][steps][pixels] (conf uint16 of that shape or None), the history [streams][pixels]; nothing is
    changed in place.  -> (filtered maps, hv', hb', stats uint32 [streams * steps][5])"""
    maps = np.ascontiguousarray(maps, np.float32)
    streams, steps, pixels = maps.shape
    out = np.empty_like(maps)
    hv, hb = hv.reshape(streams, pixels).copy(), hb.reshape(streams, pixels).copy()
    stats = np.zeros((streams * steps, 5), np.uint32)
    for s in range(streams):
        for t in range(steps):
            out[s, t], hv[s], hb[s], cls = step(spec, hv[s], hb[s], maps[s, t], None if conf is None else conf[s, t])
            stats[s * steps + t] = np.bincount(cls, minlength=5)
    return out, hv, hb, stats


def forgets(hb_before, hb_after):
    """pixels whose history forgot in a step: eight invalid inputs in a row, the last of them now"""
    return (hb_before != 0) & (hb_after == 0)
