"""Restatement of the TSDF volume contract of include/sgm_mi355x.h (sgm_volume_spec), numpy on float32 arrays: every float
operation is one IEEE float32 operation, as in the kernels; the running average is exact integer arithmetic (int64 here).  Built on
the cloud's restatement (cloud_ref.kept): the contributing pixels and their Z are the cloud's.

    spec(...)                                             -> a plain record of the volume's fields
    empty(v)                                              -> uint32 [nz][ny][nx] of zeros: the empty volume
    unpack(vox) / pack(tq, w)                             -> (tq int64, w int64) of a volume's words, and back
    centres(v)                                            -> (px [nx], py [ny], pz [nz]) float32: the voxel centres
    integrate(vox, v, src, poses, disp, mask, conf)       -> (the volume after src.frames frames, the number of updates)
    crossings(vox, v, min_weight)                         -> SURFACE records sorted by id
"""
import types

import numpy as np

import cloud_ref as CR

SURFACE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("id", np.uint32)])
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)     # the pose of a camera at the world's origin


def spec(nx, ny, nz, voxel, origin, trunc, max_weight=64):
    return types.SimpleNamespace(nx=nx, ny=ny, nz=nz, voxel=voxel, origin=tuple(float(o) for o in origin), trunc=trunc,
                                 max_weight=max_weight)


def pose(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    """[12] float32: R row-major, then t (world -> camera)"""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(np.float32)


def empty(v):
    return np.zeros((v.nz, v.ny, v.nx), np.uint32)


def unpack(vox):
    vox = np.asarray(vox, np.uint32)
    return (vox & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int64), (vox >> np.uint32(16)).astype(np.int64)


def pack(tq, w):
    return ((np.asarray(w, np.int64) << 16) | (np.asarray(tq, np.int64) & 0xFFFF)).astype(np.uint32)


def centres(v):
    f = np.float32
    return tuple(f(o) + (np.arange(n, dtype=f) + f(0.5)) * f(v.voxel) for o, n in zip(v.origin, (v.nx, v.ny, v.nz)))


def integrate(vox, v, src, poses, disp, mask=None, conf=None):
    f = np.float32
    keep, Z = CR.kept(disp, src, mask, conf)
    poses = np.asarray(poses, f).reshape(src.frames, 12)
    tq, w = unpack(np.asarray(vox).reshape(v.nz, v.ny, v.nx))
    tq, w = tq.copy(), w.copy()
    px, py, pz = centres(v)
    px, py, pz = px[None, None, :], py[None, :, None], pz[:, None, None]
    trunc = f(v.trunc)
    updates = 0
    for fr in range(src.frames):                                  # frames take effect in order
        P = poses[fr]
        with np.errstate(all="ignore"):
            Xp = ((P[0] * px + P[1] * py) + P[2] * pz) + P[9]
            Yp = ((P[3] * px + P[4] * py) + P[5] * pz) + P[10]
            Zp = ((P[6] * px + P[7] * py) + P[8] * pz) + P[11]
            ok = np.isfinite(Zp) & (Zp > 0)
            u = f(src.fx) * (Xp / Zp) + f(src.cx)
            vv = f(src.fy) * (Yp / Zp) + f(src.cy)
            ok &= np.isfinite(u) & np.isfinite(vv)
            uf, vf = np.floor(u + f(0.5)), np.floor(vv + f(0.5))
            ok &= (0 <= uf) & (uf < f(src.width)) & (0 <= vf) & (vf < f(src.height))       # in float, before any conversion
        for arr in (Xp, Zp, u, uf):
            assert arr.dtype == np.float32
        ui, vi = uf[ok].astype(np.int64), vf[ok].astype(np.int64)
        with np.errstate(all="ignore"):
            sdf = Z[fr, vi, ui] - Zp[ok]
            upd = keep[fr, vi, ui] & ~(sdf < -trunc)
            q = np.rint((np.minimum(sdf, trunc) / trunc) * f(32767))                         # round half to even
        assert sdf.dtype == np.float32 and q.dtype == np.float32
        at = tuple(a[upd] for a in np.nonzero(ok))
        num = tq[at] * w[at] + q[upd].astype(np.int64)
        den = w[at] + 1
        tq[at] = (2 * num + den) // (2 * den)                      # numpy's // floors
        w[at] = np.minimum(w[at] + 1, v.max_weight)
        updates += int(upd.sum())
    return pack(tq, w), updates


def crossings(vox, v, min_weight):
    f = np.float32
    tq, w = unpack(np.asarray(vox).reshape(v.nz, v.ny, v.nx))
    c = centres(v)
    n = np.arange(v.nx * v.ny * v.nz, dtype=np.int64).reshape(v.nz, v.ny, v.nx)
    recs = []
    for a in range(3):
        axis = 2 - a                                              # x is the fastest: the last numpy axis
        lo = tuple(slice(0, -1) if d == axis else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == axis else slice(None) for d in range(3))
        cross = (w[lo] >= min_weight) & (w[hi] >= min_weight) & ((tq[lo] < 0) != (tq[hi] < 0))
        k, j, i = np.nonzero(cross)
        tn, tm = tq[lo][cross].astype(f), tq[hi][cross].astype(f)
        with np.errstate(all="ignore"):
            s = tn / (tn - tm)
        assert s.dtype == np.float32
        rec = np.empty(i.size, SURFACE)
        rec["x"], rec["y"], rec["z"] = c[0][i], c[1][j], c[2][k]
        name = "xyz"[a]
        rec[name] = rec[name] + s * f(v.voxel)
        rec["id"] = (n[lo][cross] * 4 + a).astype(np.uint32)
        recs.append(rec)
    out = np.concatenate(recs)
    return out[np.argsort(out["id"], kind="stable")]
