"""Restatement of the tracking contract of include/sgm_mi355x.h (sgm_track_spec).  Per pixel: numpy on float32 arrays, every float
operation one IEEE float32 operation, as in the kernel; the parentheses are the header's.  The sums: Python ints.  The step: Python
floats (IEEE doubles) in explicit loops, operation for operation what csrc/sgm_host.c does.  The source is the one of
tests/cloud_ref.py.

    model(width, height, fx, fy, cx, cy, dist_max, span, iterations=1, min_pixels=6, min_pivot=0.0)  -> a plain record of the fields
    quantised(disp, s, m, pose, depth, normal, mask, conf)  -> (associated bool [H][W], q int64 [H][W][7]) of ONE frame
    sums(disp, s, m, poses, depth, normal, mask=None, conf=None)  -> int64 [frames][29]
    solve(m, sums29, pose)  -> (pose' as a list of 12 floats, dict(pixels, rms, status))
    track(disp, s, m, poses, depth, normal, mask=None, conf=None)  -> (poses float64 [frames][12], stats, trace_sums, trace_poses)
    world_pose(model_pose, rel)  -> float32 [12]
"""
import math
import types

import numpy as np

import cloud_ref as CR

PAIRS = [(i, j) for i in range(7) for j in range(i, 7)]           # row-major upper triangle of the 7 x 7 matrix
f32 = np.float32


def model(width, height, fx, fy, cx, cy, dist_max, span, iterations=1, min_pixels=6, min_pivot=0.0):
    return types.SimpleNamespace(width=width, height=height, fx=fx, fy=fy, cx=cx, cy=cy, dist_max=dist_max, span=span,
                                 iterations=iterations, min_pixels=min_pixels, min_pivot=min_pivot)


def quantised(disp, s, m, pose, depth, normal, mask=None, conf=None):
    """one frame: disp [H][W] of the source s (s.frames is not looked at), depth [mh][mw], normal [mh][mw][3], pose [12]"""
    one = types.SimpleNamespace(**dict(vars(s), frames=1))
    keep, Z = CR.kept(disp, one, mask, conf)
    X, Y = CR._xyz(one, Z)
    keep, X, Y, Z = keep[0], X[0], Y[0], Z[0]
    P = np.asarray(pose, f32).reshape(12)
    depth = np.ascontiguousarray(depth, f32).reshape(m.height, m.width)
    normal = np.ascontiguousarray(normal, f32).reshape(m.height, m.width, 3)
    fx, fy, cx, cy, dist_max, span = f32(m.fx), f32(m.fy), f32(m.cx), f32(m.cy), f32(m.dist_max), f32(m.span)
    with np.errstate(all="ignore"):
        Px = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9]
        Py = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10]
        Pz = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11]
        ok = keep & np.isfinite(Pz) & (Pz > 0)
        u = fx * (Px / Pz) + cx
        v = fy * (Py / Pz) + cy
        ok &= np.isfinite(u) & np.isfinite(v)
        uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        ok &= (uf >= 0) & (uf < f32(m.width)) & (vf >= 0) & (vf < f32(m.height))          # in float, before any conversion
        ui, vi = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
        Zm = depth[vi, ui]
        n = [normal[vi, ui, a] for a in range(3)]
        ok &= np.isfinite(Zm) & (Zm > 0) & np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2])
        e0 = ((uf - cx) * Zm) / fx - Px
        e1 = ((vf - cy) * Zm) / fy - Py
        e2 = Zm - Pz
        d2 = (e0 * e0 + e1 * e1) + e2 * e2
        ok &= np.isfinite(d2) & (d2 <= dist_max * dist_max)
        r = (n[0] * e0 + n[1] * e1) + n[2] * e2
        c0 = Py * n[2] - Pz * n[1]
        c1 = Pz * n[0] - Px * n[2]
        c2 = Px * n[1] - Py * n[0]
        val = [c0 / span, c1 / span, c2 / span, n[0], n[1], n[2], r / dist_max]
        for t in val:
            assert t.dtype == f32
            ok &= np.isfinite(t) & (np.abs(t) <= f32(8.0))
        q = np.stack([np.where(ok, np.rint(t * f32(65536.0)), 0).astype(np.int64) for t in val], axis=-1)   # rint: half to even
    return ok, q


def sums_of(ok, q):
    """the 29 sums of one frame as Python ints"""
    sel = q[ok].astype(object)                                   # Python ints: no width to overflow
    out = [int(np.sum(sel[:, i] * sel[:, j])) if len(sel) else 0 for i, j in PAIRS]
    return out + [int(ok.sum())]


def sums(disp, s, m, poses, depth, normal, mask=None, conf=None):
    disp, mask, conf = CR._maps(disp, s, mask, conf)
    poses = np.asarray(poses, f32).reshape(s.frames, 12)
    depth = np.ascontiguousarray(depth, f32).reshape(s.frames, m.height, m.width)
    normal = np.ascontiguousarray(normal, f32).reshape(s.frames, m.height, m.width, 3)
    out = []
    for f in range(s.frames):
        ok, q = quantised(disp[f], s, m, poses[f], depth[f], normal[f], None if mask is None else mask[f], None if conf is None else conf[f])
        out.append(sums_of(ok, q))
    assert all(abs(v) < 1 << 62 for row in out for v in row)
    return np.array(out, np.int64)


def _sum(sums29, i, j):
    return float(int(sums29[i * 7 - i * (i - 1) // 2 + (j - i)]))


def solve(m, sums29, pose):
    """sgm_track_solve: (pose', stats)"""
    pose = [float(x) for x in np.asarray(pose, np.float64).reshape(12)]
    dist_max, span, min_pivot = float(f32(m.dist_max)), float(f32(m.span)), float(f32(m.min_pivot))
    pixels = int(sums29[28])
    rms = dist_max * math.sqrt(float(int(sums29[27])) / float(pixels)) / 65536.0 if pixels > 0 else 0.0
    stats = dict(pixels=pixels, rms=rms, status=0)
    if pixels < m.min_pixels:
        stats["status"] = 1
        return pose, stats
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        Ajj = _sum(sums29, j, j)
        acc = 0.0
        for k in range(j):
            acc += (L[j][k] * L[j][k]) * D[k]
        D[j] = Ajj - acc
        if not math.isfinite(D[j]) or not D[j] > min_pivot * Ajj:
            stats["status"] = 2
            return pose, stats
        for i in range(j + 1, 6):
            acc = 0.0
            for k in range(j):
                acc += (L[i][k] * L[j][k]) * D[k]
            L[i][j] = (_sum(sums29, j, i) - acc) / D[j]
    y, xi = [0.0] * 6, [0.0] * 6
    for i in range(6):
        acc = 0.0
        for k in range(i):
            acc += L[i][k] * y[k]
        y[i] = _sum(sums29, i, 6) - acc
    for i in range(5, -1, -1):
        acc = 0.0
        for k in range(i + 1, 6):
            acc += L[k][i] * xi[k]
        xi[i] = y[i] / D[i] - acc
    if not all(math.isfinite(x) for x in xi):
        stats["status"] = 2
        return pose, stats
    k = dist_max / span
    s = [(xi[i] * k) * 0.5 for i in range(3)]
    v = [xi[3 + i] * dist_max for i in range(3)]
    ss = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
    a, den = 1.0 - ss, 1.0 + ss
    X = [[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]]
    Ri = [[((a * (1.0 if r == c else 0.0) + 2.0 * (s[r] * s[c])) + 2.0 * X[r][c]) / den for c in range(3)] for r in range(3)]
    out = [0.0] * 12
    for r in range(3):
        for c in range(3):
            out[3 * r + c] = (Ri[r][0] * pose[c] + Ri[r][1] * pose[3 + c]) + Ri[r][2] * pose[6 + c]
        out[9 + r] = ((Ri[r][0] * pose[9] + Ri[r][1] * pose[10]) + Ri[r][2] * pose[11]) + v[r]
    if not all(math.isfinite(x) for x in out):
        stats["status"] = 2
        return pose, stats
    return out, stats


def track(disp, s, m, poses, depth, normal, mask=None, conf=None):
    """sgm_track: m.iterations rounds; the kernel's poses are the doubles rounded once to float32; a frame whose solve fails keeps
    its pose and its status and sits out the remaining rounds (its sums are still those of the pose it kept)."""
    poses = np.array(poses, np.float64).reshape(s.frames, 12)
    stats = [dict(pixels=0, rms=0.0, status=0) for _ in range(s.frames)]
    out = [False] * s.frames
    trace_sums, trace_poses = [], [poses.copy()]
    for _ in range(m.iterations):
        got = sums(disp, s, m, poses.astype(f32), depth, normal, mask, conf)
        trace_sums.append(got)
        for f in range(s.frames):
            if out[f]:
                continue
            nxt, stats[f] = solve(m, got[f], poses[f])
            if stats[f]["status"] != 0:
                out[f] = True
            else:
                poses[f] = nxt
        trace_poses.append(poses.copy())
    return poses, stats, np.stack(trace_sums), np.stack(trace_poses)


def world_pose(model_pose, rel):
    """sgm_track_world_pose: rel^-1 o model_pose, in double, rounded once"""
    m = [float(x) for x in np.asarray(model_pose, f32).reshape(12)]
    r = [float(x) for x in np.asarray(rel, np.float64).reshape(12)]
    dt = [m[9] - r[9], m[10] - r[10], m[11] - r[11]]
    out = [0.0] * 12
    for a in range(3):
        for c in range(3):
            out[3 * a + c] = (r[a] * m[c] + r[3 + a] * m[3 + c]) + r[6 + a] * m[6 + c]
        out[9 + a] = (r[a] * dt[0] + r[3 + a] * dt[1]) + r[6 + a] * dt[2]
    return np.array(out, np.float64).astype(f32)
