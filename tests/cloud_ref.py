"""Restatement of the point-cloud contract of include/sgm_mi355x.h (sgm_cloud_spec), numpy on float32 arrays: every operation is
one IEEE float32 operation, as in the kernels.

    spec(...)                               -> a plain record of the twelve fields (any object with those attributes serves)
    kept(disp, spec, mask=None, conf=None)  -> (keep bool, Z float32) of the map's shape [frames][H][W]
    organized(disp, spec, mask, conf)       -> float32 [frames][H][W][3]: X Y Z of the kept pixels, NaN 0x7FC00000 elsewhere
    points(disp, spec, mask, conf)          -> (records POINT, offsets uint32 [frames + 1]) in raster order
"""
import types

import numpy as np

POINT = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("pixel", np.uint32)])
QNAN = np.uint32(0x7FC00000)


def spec(width, height, fx, fy, cx, cy, baseline, doffs=0.0, frames=1, z_min=0.0, z_max=np.inf, min_conf=0):
    return types.SimpleNamespace(width=width, height=height, frames=frames, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs,
                                 z_min=z_min, z_max=z_max, min_conf=min_conf)


def fb_of(s):
    """(float)((double)fx * (double)baseline): one rounding of the exact product"""
    return np.float32(np.float64(np.float32(s.fx)) * np.float64(np.float32(s.baseline)))


def _maps(disp, s, mask, conf):
    shape = (s.frames, s.height, s.width)
    d = np.ascontiguousarray(disp, np.float32).reshape(shape)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(shape)
    k = None if conf is None else np.ascontiguousarray(conf, np.uint16).reshape(shape)
    return d, m, k


def kept(disp, s, mask=None, conf=None):
    d, m, k = _maps(disp, s, mask, conf)
    with np.errstate(all="ignore"):
        den = d + np.float32(s.doffs)
        Z = fb_of(s) / den
        keep = np.isfinite(d) & np.isfinite(den) & (den > 0) & np.isfinite(Z) & (np.float32(s.z_min) <= Z) & (Z <= np.float32(s.z_max))
    if m is not None:
        keep &= m != 0
    if k is not None:
        keep &= k.astype(np.uint32) >= np.uint32(s.min_conf)
    assert Z.dtype == np.float32
    return keep, Z


def _xyz(s, Z):
    x = np.arange(s.width, dtype=np.float32)[None, None, :]
    y = np.arange(s.height, dtype=np.float32)[None, :, None]
    with np.errstate(all="ignore"):
        X = ((x - np.float32(s.cx)) * Z) / np.float32(s.fx)
        Y = ((y - np.float32(s.cy)) * Z) / np.float32(s.fy)
    assert X.dtype == np.float32 and Y.dtype == np.float32
    return X, Y


def organized(disp, s, mask=None, conf=None):
    keep, Z = kept(disp, s, mask, conf)
    X, Y = _xyz(s, Z)
    out = np.full(keep.shape + (3,), QNAN, np.uint32)
    for c, v in enumerate((X, Y, Z)):
        out[..., c][keep] = v.view(np.uint32)[keep]
    return out.view(np.float32)


def points(disp, s, mask=None, conf=None):
    keep, Z = kept(disp, s, mask, conf)
    X, Y = _xyz(s, Z)
    f, y, x = np.nonzero(keep)                                   # raster order: frame-major, then row, then column
    rec = np.empty(f.size, POINT)
    rec["x"], rec["y"], rec["z"] = X[f, y, x], Y[f, y, x], Z[f, y, x]
    rec["pixel"] = (y.astype(np.uint32) << np.uint32(16)) | x.astype(np.uint32)
    offsets = np.zeros(s.frames + 1, np.uint32)
    offsets[1:] = np.cumsum(keep.reshape(s.frames, -1).sum(axis=1))
    return rec, offsets
