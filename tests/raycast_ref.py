"""Restatement of the ray-cast contract of include/sgm_mi355x.h (sgm_raycast_spec), numpy on float32 arrays: every float operation
is one IEEE float32 operation, as in the kernel; the parentheses are the header's.  The volume is the one of tests/volume_ref.py.

    view(width, height, fx, fy, cx, cy, z_min, z_max, step, min_weight=1, frames=1)   -> a plain record of the view's fields
    raycast(vox, v, view, poses)   -> (depth [frames][height][width] float32, normal [frames][height][width][3] float32, stats)

Empty pixels and refused normals hold the quiet NaN 0x7FC00000.  stats counts, over all frames, what the march met: "hits" (front
hits whose refinement succeeded), "back" (back faces), "refine_failed" (front hits whose refinement failed), "normals" (valid
normals).
"""
import types

import numpy as np

import volume_ref as VR

QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def view(width, height, fx, fy, cx, cy, z_min, z_max, step, min_weight=1, frames=1):
    return types.SimpleNamespace(width=width, height=height, frames=frames, fx=fx, fy=fy, cx=cx, cy=cy, z_min=z_min, z_max=z_max,
                                 step=step, min_weight=min_weight)


def _nearest(tq, w, dims, min_weight, g):
    """the nearest sample at g ([3] arrays): (valid, negative)"""
    f = np.float32
    ok = np.ones(g[0].shape, bool)
    for a in range(3):
        ok &= np.isfinite(g[a])
        with np.errstate(invalid="ignore"):
            ok &= (g[a] >= 0) & (g[a] < f(dims[a]))               # in float, before any conversion
    at = [np.where(ok, np.floor(g[a]), 0).astype(np.int64) for a in range(3)]
    ok &= w[at[2], at[1], at[0]] >= min_weight
    return ok, ok & (tq[at[2], at[1], at[0]] < 0)


def _lerp(p, q, s):
    return p + s * (q - p)


def _trilinear(tq, w, dims, min_weight, g):
    """F(g): (value float32, valid)"""
    f = np.float32
    ok = np.ones(g[0].shape, bool)
    i0, fr = [], []
    for a in range(3):
        with np.errstate(invalid="ignore", over="ignore"):
            h = g[a] - f(0.5)
            ok &= np.isfinite(h)
            lo = np.floor(h)
            ok &= (lo >= 0) & (lo + f(1.0) < f(dims[a]))          # in float
            fr.append(h - lo)
        i0.append(lo)
    at = [np.where(ok, i0[a], 0).astype(np.int64) for a in range(3)]
    hi = [np.minimum(at[a] + 1, dims[a] - 1) for a in range(3)]   # (only read where ok, where at + 1 is inside)
    t = {}
    for dz, z in enumerate((at[2], hi[2])):
        for dy, y in enumerate((at[1], hi[1])):
            for dx, x in enumerate((at[0], hi[0])):
                ok &= w[z, y, x] >= min_weight
                t[dx, dy, dz] = tq[z, y, x].astype(f)
    with np.errstate(invalid="ignore"):
        c = {(dy, dz): _lerp(t[0, dy, dz], t[1, dy, dz], fr[0]) for dy in (0, 1) for dz in (0, 1)}        # along x first
        c = {dz: _lerp(c[0, dz], c[1, dz], fr[1]) for dz in (0, 1)}                                        # then y
        F = _lerp(c[0], c[1], fr[2])                                                                        # then z
    assert F.dtype == np.float32
    return F, ok


def raycast(vox, v, vw, poses):
    f = np.float32
    dims = (v.nx, v.ny, v.nz)
    tq, w = VR.unpack(np.asarray(vox).reshape(v.nz, v.ny, v.nx))
    poses = np.asarray(poses, f).reshape(vw.frames, 12)
    fx, fy, cx, cy, z_min, z_max, step, voxel = (f(t) for t in (vw.fx, vw.fy, vw.cx, vw.cy, vw.z_min, vw.z_max, vw.step, v.voxel))
    origin = [f(o) for o in v.origin]
    depth = np.full((vw.frames, vw.height, vw.width), QNAN, f)
    normal = np.full((vw.frames, vw.height, vw.width, 3), QNAN, f)
    stats = dict(hits=0, back=0, refine_failed=0, normals=0)
    a = ((np.arange(vw.width, dtype=f) - cx) / fx)[None, :]
    b = ((np.arange(vw.height, dtype=f) - cy) / fy)[:, None]
    shape = (vw.height, vw.width)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for fr in range(vw.frames):
            R, t = poses[fr, :9].reshape(3, 3), poses[fr, 9:]
            go, gd = [], []
            for i in range(3):
                c = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
                d = np.broadcast_to((R[0, i] * a + R[1, i] * b) + R[2, i], shape)
                go.append(np.broadcast_to((c - origin[i]) / voxel, shape))
                gd.append(d / voxel)
            g_of = lambda Z, sel=slice(None): [go[i][sel] + Z * gd[i][sel] for i in range(3)]
            # the march: 0 no previous sample, 1 valid and non-negative, 2 valid and negative
            prev = np.zeros(shape, np.int8)
            active = np.ones(shape, bool)
            front = np.zeros(shape, bool)
            hit_k = np.zeros(shape, np.int64)
            k = 0
            while True:
                Z = z_min + f(k) * step
                assert Z.dtype == np.float32
                if not Z <= z_max:
                    break
                ok, neg = _nearest(tq, w, dims, vw.min_weight, g_of(Z))
                cur = np.where(ok, np.where(neg, 2, 1), 0).astype(np.int8)
                now_front = active & (prev == 1) & (cur == 2)
                now_back = active & (prev == 2) & (cur == 1)
                front |= now_front
                hit_k[now_front] = k
                stats["back"] += int(now_back.sum())
                active &= ~(now_front | now_back)
                prev = cur
                k += 1
                if not active.any():
                    break
            sel = np.nonzero(front)
            if sel[0].size == 0:
                continue
            Zc = z_min + hit_k[sel].astype(f) * step
            Zp = z_min + (hit_k[sel] - 1).astype(f) * step
            Fp, okp = _trilinear(tq, w, dims, vw.min_weight, g_of(Zp, sel))
            Fc, okc = _trilinear(tq, w, dims, vw.min_weight, g_of(Zc, sel))
            den = Fp - Fc
            good = okp & okc & (den > 0)
            s = np.minimum(np.maximum(Fp / np.where(good, den, f(1.0)), f(0.0)), f(1.0))
            Zs = Zp + s * step
            assert Zs.dtype == np.float32
            stats["hits"] += int(good.sum())
            stats["refine_failed"] += int((~good).sum())
            sel = tuple(x[good] for x in sel)
            Zs = Zs[good]
            depth[fr][sel] = Zs
            gs = g_of(Zs, sel)
            nw, nok = [], np.ones(Zs.shape, bool)
            for ax in range(3):
                up = [gs[i] + f(1.0) if i == ax else gs[i] for i in range(3)]
                dn = [gs[i] - f(1.0) if i == ax else gs[i] for i in range(3)]
                Fu, oku = _trilinear(tq, w, dims, vw.min_weight, up)
                Fd, okd = _trilinear(tq, w, dims, vw.min_weight, dn)
                nw.append(Fu - Fd)
                nok &= oku & okd
            n = [(R[r, 0] * nw[0] + R[r, 1] * nw[1]) + R[r, 2] * nw[2] for r in range(3)]
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            assert length.dtype == np.float32
            nok &= np.isfinite(length) & (length > 0)
            stats["normals"] += int(nok.sum())
            out = np.stack([np.where(nok, n[r] / np.where(nok, length, f(1.0)), QNAN) for r in range(3)], axis=-1).astype(f)
            normal[fr][sel] = out
    return depth, normal, stats
