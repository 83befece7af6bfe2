"""Numpy restatement of the hole filling (include/sgm_mi355x.h, SGM_SetFillHoles) -- TEST INFRASTRUCTURE ONLY.

Parity unpinned by the reference (it has no such step): this module is the checker the device is held to, bit for bit.
Vectorised per direction and step over the target pixels, so that a KITTI-sized frame takes seconds.

    classify(ref, oth, thres, right, check)   u8 classes 0 valid / 1 occluded / 2 mismatched
    fill(disp, cls, R)                        the three Jacobi passes ([H][W] or [B][H][W]; cls None = pass 3 alone)
    expected(stages, opt, right, oracle)      classes, filled map and final map from the oracle's stages 4, 5 and 7
"""
from __future__ import annotations

import numpy as np

INF = np.float32(np.inf)
# (dx, dy) of the 8 rays
RAYS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]


def _round_col(x, d):
    """(int)((double)((float)x +- d) + 0.5): float32 sum, double add, truncation toward zero (the LR check's rounding)."""
    return ((x.astype(np.float32) + d).astype(np.float64) + 0.5).astype(np.int64)


def classify(ref, oth, thres, right=False, check=True):
    """Class map of one frame from the reference view's WTA map `ref` and the other view's `oth` (before the LR check)."""
    ref = np.asarray(ref, np.float32)
    oth = np.asarray(oth, np.float32)
    h, w = ref.shape
    cls = np.zeros((h, w), np.uint8)
    if not check:
        return cls
    ys, xs = np.mgrid[0:h, 0:w]
    fin = ref != INF
    cls[~fin] = 2
    d = np.where(fin, ref, np.float32(0))
    sgn = np.float32(1) if right else np.float32(-1)
    xo = _round_col(xs, sgn * d)                                  # x + d (right view) or x - d (left view), in float32
    inb = fin & (xo >= 0) & (xo < w)
    cls[fin & ~inb] = 2
    o = np.full((h, w), INF, np.float32)
    o[inb] = oth[ys[inb], xo[inb]]
    differ = inb & (o != INF)
    differ &= np.abs((d - np.where(differ, o, np.float32(0))).astype(np.float64)) > np.float64(np.float32(thres))
    xb = np.zeros((h, w), np.int64)
    xb[differ] = _round_col(xo[differ], -sgn * o[differ])          # back into the reference view
    back_in = differ & (xb >= 0) & (xb < w)
    occluded = np.zeros((h, w), bool)
    occluded[back_in] = ref[ys[back_in], xb[back_in]] > d[back_in]
    cls[differ] = 2
    cls[occluded] = 1
    return cls


def _candidates(m, ty, tx, R):
    """[8][n] first finite value along each ray of the targets (ty, tx) within R steps of frame m; INF = none."""
    h, w = m.shape
    out = np.full((8, ty.size), INF, np.float32)
    for k, (dx, dy) in enumerate(RAYS):
        active = np.arange(ty.size)
        for step in range(1, R + 1):
            if active.size == 0:
                break
            yy = ty[active] + dy * step
            xx = tx[active] + dx * step
            inb = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            active, yy, xx = active[inb], yy[inb], xx[inb]
            v = m[yy, xx]
            hit = v != INF
            out[k, active[hit]] = v[hit]
            active = active[~hit]
    return out


def _pass(m, targets, R, background):
    ty, tx = np.nonzero(targets)
    res = m.copy()
    if ty.size == 0:
        return res
    s = np.sort(_candidates(m, ty, tx, R), axis=0)               # INF (no candidate) sorts last
    k = (s != INF).sum(axis=0)
    pick = np.where(k >= 2, 1, 0) if background else k // 2
    res[ty, tx] = s[pick, np.arange(ty.size)]
    return res


def fill_frame(disp, cls, R):
    m = np.array(disp, np.float32, copy=True)
    if cls is not None:
        m = _pass(m, (m == INF) & (cls == 1), R, True)
        m = _pass(m, (m == INF) & (cls == 2), R, False)
    return _pass(m, m == INF, R, False)


def fill(disp, cls, R):
    """The three passes on one map [H][W] or on each frame of [B][H][W] (a walk stops at its frame's edge)."""
    disp = np.asarray(disp, np.float32)
    if disp.ndim == 2:
        return fill_frame(disp, cls, R)
    return np.stack([fill_frame(disp[f], None if cls is None else cls[f], R) for f in range(disp.shape[0])])


def expected(st, opt, oracle, right=False):
    """(classes, filled, final) of one frame from the oracle's stage dict (Oracle.run / Oracle.stages)."""
    ref, oth = (st["disp_r"], st["disp_l"]) if right else (st["disp_l"], st["disp_r"])
    cls = classify(ref, oth, opt.lrcheck_thres, right=right, check=bool(opt.is_check_lr))
    filled = fill(st["after_speckle"], cls, int(opt.max_disparity))
    return cls, filled, oracle.median(filled)
