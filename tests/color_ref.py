"""Restatement of the colour section of include/sgm_mi355x.h, numpy on float32 arrays: every float operation is one IEEE float32
operation, as in the kernels; the averages are exact integer arithmetic (int64 here).  Built on the volume's and the ray-cast's
restatements (volume_ref, raycast_ref): the TSDF words, the depth and the normals are theirs.

    empty(v)                                              -> uint32 [nz][ny][nx] of zeros: no colour anywhere
    unpack(col) / pack(r, g, b, cw)                       -> the four bytes of the colour words as int64, and back
    pixels(image, channels)                               -> (r, g, b) int64 [frames][height][width] of an image as the call takes it
    integrate(vox, col, v, src, poses, disp, mask, conf, image, channels)
                                                          -> (the volume, the colours, stats) after src.frames frames
    raycast(vox, col, v, view, poses)                     -> (depth, normal, rgba uint32 [frames][height][width], stats)
    colors(vox, col, v, ids, id_kinds)                    -> uint32 [len(ids)]: the colour of every record id

stats of integrate: "updates" (TSDF updates), "colored" (colour updates), "halves" (colour updates in which a channel met an exact
half, 2*rem == den).  stats of raycast: the ray-cast's own and the pixel classes "trilinear", "nearest", "uncolored" (a hit
without colour), "empty".  CLASSES of colors(): see color_classes().
"""
import numpy as np

import cloud_ref as CR
import mesh_ref as MR
import raycast_ref as RR
import volume_ref as VR

ALPHA = 0xFF000000


def empty(v):
    return np.zeros((v.nz, v.ny, v.nx), np.uint32)


def unpack(col):
    col = np.asarray(col, np.uint32).astype(np.int64)
    return col & 0xFF, (col >> 8) & 0xFF, (col >> 16) & 0xFF, col >> 24


def pack(r, g, b, cw):
    return ((np.asarray(cw, np.int64) << 24) | (np.asarray(b, np.int64) << 16) | (np.asarray(g, np.int64) << 8) | np.asarray(r, np.int64)).astype(np.uint32)


def pixels(image, channels):
    if channels == 1:
        p = np.asarray(image, np.uint8).astype(np.int64)
        return p, p, p
    assert channels == 4
    p = np.asarray(image, np.uint32).astype(np.int64)
    return p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF           # the top byte is ignored


def integrate(vox, col, v, src, poses, disp, mask, conf, image, channels):
    """volume_ref.integrate with the colour words carried along (the geometry is restated here line by line, so that the colour's
    condition can name sdf; tests/test_color_cpu.py holds the TSDF words against volume_ref.integrate)"""
    f = np.float32
    keep, Z = CR.kept(disp, src, mask, conf)
    poses = np.asarray(poses, f).reshape(src.frames, 12)
    shape = (v.nz, v.ny, v.nx)
    tq, w = VR.unpack(np.asarray(vox).reshape(shape))
    tq, w = tq.copy(), w.copy()
    c = [a.copy() for a in unpack(np.asarray(col).reshape(shape))]
    cw = c.pop()
    p = [np.asarray(a).reshape(src.frames, src.height, src.width) for a in pixels(image, channels)]
    px, py, pz = VR.centres(v)
    px, py, pz = px[None, None, :], py[None, :, None], pz[:, None, None]
    trunc = f(v.trunc)
    cap = min(v.max_weight, 255)
    stats = dict(updates=0, colored=0, halves=0)
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
        assert Zp.dtype == np.float32 and uf.dtype == np.float32
        ui, vi = uf[ok].astype(np.int64), vf[ok].astype(np.int64)
        with np.errstate(all="ignore"):
            sdf = Z[fr, vi, ui] - Zp[ok]
            upd = keep[fr, vi, ui] & ~(sdf < -trunc)
            q = np.rint((np.minimum(sdf, trunc) / trunc) * f(32767))
            paint = upd & (sdf <= trunc)                          # far in front of the surface: distance, no colour
        assert sdf.dtype == np.float32
        at = tuple(a[upd] for a in np.nonzero(ok))
        num = tq[at] * w[at] + q[upd].astype(np.int64)
        den = w[at] + 1
        tq[at] = (2 * num + den) // (2 * den)
        w[at] = np.minimum(w[at] + 1, v.max_weight)
        stats["updates"] += int(upd.sum())
        at = tuple(a[paint] for a in np.nonzero(ok))
        den = cw[at] + 1
        half = np.zeros(den.shape, bool)
        for ch in range(3):
            num = c[ch][at] * cw[at] + p[ch][fr, vi[paint], ui[paint]]
            half |= 2 * (num % den) == den
            c[ch][at] = (2 * num + den) // (2 * den)
        cw[at] = np.minimum(cw[at] + 1, cap)
        stats["colored"] += int(paint.sum())
        stats["halves"] += int(half.sum())
    return VR.pack(tq, w), pack(c[0], c[1], c[2], cw), stats


def _lerp(p, q, s):
    return p + s * (q - p)


def raycast(vox, col, v, vw, poses):
    f = np.float32
    dims = (v.nx, v.ny, v.nz)
    depth, normal, stats = RR.raycast(vox, v, vw, poses)
    r, g, b, cw = unpack(np.asarray(col).reshape(v.nz, v.ny, v.nx))
    chans = (r, g, b)
    poses = np.asarray(poses, f).reshape(vw.frames, 12)
    fx, fy, cx, cy, voxel = (f(t) for t in (vw.fx, vw.fy, vw.cx, vw.cy, v.voxel))
    origin = [f(o) for o in v.origin]
    rgba = np.zeros((vw.frames, vw.height, vw.width), np.uint32)
    stats = dict(stats, trilinear=0, nearest=0, uncolored=0, empty=0)
    a = ((np.arange(vw.width, dtype=f) - cx) / fx)[None, :]
    bb = ((np.arange(vw.height, dtype=f) - cy) / fy)[:, None]
    shape = (vw.height, vw.width)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for fr in range(vw.frames):
            R, t = poses[fr, :9].reshape(3, 3), poses[fr, 9:]
            hit = np.isfinite(depth[fr])
            stats["empty"] += int((~hit).sum())
            sel = np.nonzero(hit)
            if sel[0].size == 0:
                continue
            Zs = depth[fr][sel]
            gs = []
            for i in range(3):                                    # g* = go + Z* * gd, as the ray-cast's contract has them
                c = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
                d = np.broadcast_to((R[0, i] * a + R[1, i] * bb) + R[2, i], shape)
                go = np.broadcast_to((c - origin[i]) / voxel, shape)
                gd = d / voxel
                gs.append(go[sel] + Zs * gd[sel])
                assert gs[-1].dtype == np.float32
            # trilinear: the eight voxels of F(g*)
            ok = np.ones(Zs.shape, bool)
            i0, frac = [], []
            for ax in range(3):
                h = gs[ax] - f(0.5)
                ok &= np.isfinite(h)
                lo = np.floor(h)
                ok &= (lo >= 0) & (lo + f(1.0) < f(dims[ax]))     # in float
                frac.append(h - lo)
                i0.append(lo)
            at = [np.where(ok, i0[ax], 0).astype(np.int64) for ax in range(3)]
            hi = [np.minimum(at[ax] + 1, dims[ax] - 1) for ax in range(3)]
            for z in (at[2], hi[2]):
                for y in (at[1], hi[1]):
                    for x in (at[0], hi[0]):
                        ok &= cw[z, y, x] >= 1
            out = np.zeros(Zs.shape, np.int64)
            for ch in range(3):
                t8 = {(dx, dy, dz): chans[ch][z, y, x].astype(f) for dz, z in enumerate((at[2], hi[2])) for dy, y in enumerate((at[1], hi[1]))
                      for dx, x in enumerate((at[0], hi[0]))}
                c2 = {(dy, dz): _lerp(t8[0, dy, dz], t8[1, dy, dz], frac[0]) for dy in (0, 1) for dz in (0, 1)}     # along x first
                c1 = {dz: _lerp(c2[0, dz], c2[1, dz], frac[1]) for dz in (0, 1)}                                    # then y
                value = _lerp(c1[0], c1[1], frac[2])                                                                # then z
                assert value.dtype == np.float32
                out |= np.rint(np.minimum(np.maximum(np.where(ok, value, f(0)), f(0)), f(255))).astype(np.int64) << (8 * ch)
            tri = ok
            # nearest: the voxel g* lies in, under the march's admission test
            ok = np.ones(Zs.shape, bool)
            for ax in range(3):
                ok &= np.isfinite(gs[ax]) & (gs[ax] >= 0) & (gs[ax] < f(dims[ax]))
            at = [np.where(ok, np.floor(gs[ax]), 0).astype(np.int64) for ax in range(3)]
            near = ~tri & ok & (cw[at[2], at[1], at[0]] >= 1)
            word = sum(chans[ch][at[2], at[1], at[0]] << (8 * ch) for ch in range(3))
            res = np.where(tri, out | ALPHA, np.where(near, word | ALPHA, 0)).astype(np.uint32)
            rgba[fr][sel] = res
            stats["trilinear"] += int(tri.sum())
            stats["nearest"] += int(near.sum())
            stats["uncolored"] += int((~tri & ~near).sum())
    return depth, normal, rgba, stats


def _edges(v, ids, id_kinds):
    """(valid, n, m) of the record ids: the edge's two voxels (0 where it is not valid)"""
    assert id_kinds in (4, 8)
    ids = np.asarray(ids, np.uint32).astype(np.int64)
    n, e = ids // id_kinds, ids % id_kinds
    total = v.nx * v.ny * v.nz
    valid = (n < total) & (e < id_kinds - 1)
    n, e = np.where(valid, n, 0), np.where(valid, e, 0)
    kinds = np.array(MR.KINDS, np.int64)                          # (dx, dy, dz) of edge kind e; kinds 0..2 are the axes
    i, j, k = n % v.nx, (n // v.nx) % v.ny, n // (v.nx * v.ny)
    mi, mj, mk = i + kinds[e, 0], j + kinds[e, 1], k + kinds[e, 2]
    valid &= (mi < v.nx) & (mj < v.ny) & (mk < v.nz)
    m = np.where(valid, (mk * v.ny + mj) * v.nx + mi, 0)
    return valid, np.where(valid, n, 0), m


def color_classes(vox, col, v, ids, id_kinds):
    """per record: 0 invalid edge, 1 neither end has colour, 2 exactly one, 3 both"""
    valid, n, m = _edges(v, ids, id_kinds)
    cw = unpack(col)[3].reshape(-1)
    return np.where(valid, 1 + (cw[n] >= 1).astype(np.int64) + (cw[m] >= 1), 0)


def colors(vox, col, v, ids, id_kinds):
    f = np.float32
    valid, n, m = _edges(v, ids, id_kinds)
    tq = VR.unpack(np.asarray(vox).reshape(-1))[0]
    r, g, b, cw = (a.reshape(-1) for a in unpack(col))
    tn, tm = tq[n].astype(f), tq[m].astype(f)
    den = tn - tm
    with np.errstate(all="ignore"):
        s = np.where(den != 0, np.minimum(np.maximum(tn / np.where(den != 0, den, f(1)), f(0)), f(1)), f(0)).astype(f)
    has_n, has_m = valid & (cw[n] >= 1), valid & (cw[m] >= 1)
    out = np.zeros(n.shape, np.int64)
    for ch, c in enumerate((r, g, b)):
        value = _lerp(c[n].astype(f), c[m].astype(f), s)
        assert value.dtype == np.float32
        both = np.rint(value).astype(np.int64)
        out |= np.where(has_n & has_m, both, np.where(has_n, c[n], np.where(has_m, c[m], 0))) << (8 * ch)
    return np.where(has_n | has_m, out | ALPHA, 0).astype(np.uint32)
