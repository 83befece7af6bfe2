"""Restatement of the registration contract of include/sgm_mi355x.h (sgm_register_spec), numpy on float32 arrays: every operation is
one IEEE float32 operation, as in the kernels.  Built on the cloud's restatement (cloud_ref.kept / _xyz): the contributing pixels
and their X Y Z are the cloud's.

    spec(...)                                        -> a plain record of the target's fields (any object with those attributes serves)
    spec_raw(K, dist, R, width, height, splat)       -> the target "back into the raw camera", as sgm_register_spec_raw makes it
    project(disp, src, dst, mask=None, conf=None)    -> (ok bool, Z' float32, u float32, v float32) of the map's shape
    register(disp, src, dst, mask=None, conf=None)   -> (depth float32, source uint32), [frames][dst.height][dst.width] each
    gather(source, values, fill)                     -> values carried into the target through source
"""
import types

import numpy as np

import cloud_ref as CR

QNAN = np.uint32(0x7FC00000)
NONE = np.uint32(0xFFFFFFFF)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def spec(width, height, fx, fy, cx, cy, dist=(0.0,) * 5, R=IDENTITY, t=(0.0,) * 3, z_min=0.0, z_max=np.inf, splat=2):
    return types.SimpleNamespace(width=width, height=height, fx=fx, fy=fy, cx=cx, cy=cy, dist=tuple(float(v) for v in dist),
                                 R=tuple(float(v) for v in np.asarray(R, np.float64).reshape(9)), t=tuple(float(v) for v in t),
                                 z_min=z_min, z_max=z_max, splat=splat)


def spec_raw(K, dist, R, width, height, splat=2):
    """every value computed in double and rounded once to float32; R is the transpose of the rectifying rotation"""
    K, R = (np.asarray(m, np.float64).reshape(3, 3) for m in (K, R))
    f = lambda v: float(np.float32(v))
    return spec(width, height, f(K[0, 0]), f(K[1, 1]), f(K[0, 2]), f(K[1, 2]), [f(v) for v in np.asarray(dist, np.float64).reshape(5)],
                [f(v) for v in R.T.reshape(9)], (0.0, 0.0, 0.0), 0.0, np.inf, splat)


def project(disp, s, r, mask=None, conf=None):
    """the chain of the header up to (u, v): ok = kept by the cloud's predicate and not dropped on the way"""
    keep, Z = CR.kept(disp, s, mask, conf)
    X, Y = CR._xyz(s, Z)
    f = np.float32
    R, t = [f(v) for v in r.R], [f(v) for v in r.t]
    k1, k2, p1, p2, k3 = (f(v) for v in r.dist)
    two = f(2)
    with np.errstate(all="ignore"):
        Xp = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        Yp = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        Zp = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        ok = keep & np.isfinite(Zp) & (Zp > 0) & (f(r.z_min) <= Zp) & (Zp <= f(r.z_max))
        a, b = Xp / Zp, Yp / Zp
        aa, bb, ab = a * a, b * b, a * b
        r2 = aa + bb
        rad = ((k3 * r2 + k2) * r2 + k1) * r2 + f(1)
        xd = (a * rad + (two * p1) * ab) + p2 * (r2 + two * aa)
        yd = (b * rad + p1 * (r2 + two * bb)) + (two * p2) * ab
        u = f(r.fx) * xd + f(r.cx)
        v = f(r.fy) * yd + f(r.cy)
        ok &= np.isfinite(u) & np.isfinite(v)
    for arr in (Xp, Zp, a, rad, xd, u, v):
        assert arr.dtype == np.float32
    return ok, Zp, u, v


def candidates(u, v, splat):
    """the target pixels of a projection, as float32 arrays, in the header's order"""
    f = np.float32
    with np.errstate(all="ignore"):
        if splat == 1:
            return [(np.floor(u + f(0.5)), np.floor(v + f(0.5)))]
        u0, v0 = np.floor(u), np.floor(v)
        u1, v1 = u0 + f(1), v0 + f(1)
    return [(u0, v0), (u1, v0), (u0, v1), (u1, v1)]


def keys_of(disp, s, r, mask=None, conf=None):
    """uint64 [frames][height * width] of the target: the z-buffer after every admitted candidate voted, EMPTY where none did;
    and the number of admitted candidates"""
    ok, Zp, u, v = project(disp, s, r, mask, conf)
    w, h = int(r.width), int(r.height)
    x = np.arange(s.width, dtype=np.uint64)[None, None, :]
    y = np.arange(s.height, dtype=np.uint64)[None, :, None]
    key = (Zp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.broadcast_to((y << np.uint64(16)) | x, Zp.shape)
    keys = np.full((s.frames, h * w), EMPTY, np.uint64)
    votes = 0
    for uf, vf in candidates(u, v, r.splat):
        with np.errstate(all="ignore"):
            adm = ok & (0 <= uf) & (uf < np.float32(w)) & (0 <= vf) & (vf < np.float32(h))      # in float, before any conversion
        fi = np.nonzero(adm)[0]
        at = vf[adm].astype(np.int64) * w + uf[adm].astype(np.int64)
        np.minimum.at(keys, (fi, at), key[adm])
        votes += int(adm.sum())
    return keys, votes


def register(disp, s, r, mask=None, conf=None):
    keys, _ = keys_of(disp, s, r, mask, conf)
    hit = keys != EMPTY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), QNAN)
    source = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), NONE)
    shape = (s.frames, int(r.height), int(r.width))
    return depth.reshape(shape).view(np.float32), source.reshape(shape)


def gather(source, values, fill):
    """out[f][v][u] = source == NONE ? fill : values[f][y][x]"""
    values = np.asarray(values)
    hit = source != NONE
    y, x = (source >> np.uint32(16)).astype(np.int64), (source & np.uint32(0xFFFF)).astype(np.int64)
    fi = np.broadcast_to(np.arange(source.shape[0])[:, None, None], source.shape)
    out = np.full(source.shape, fill, values.dtype)
    out[hit] = values[fi[hit], y[hit], x[hit]]
    return out
