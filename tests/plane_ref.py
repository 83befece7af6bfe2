"""Planes in a point list, restated in numpy from the contract in include/sgm_mi355x.h (sgm_plane_spec): candidates, votes, best,
sums, labels in float32 / int64 with the header's parentheses, the solve and the fit in float64 (Python floats, one operation at a
time).  Tolerance 0 against the library.

    spec(hypotheses, dist, span, ...)                       the sgm_plane_spec as a namespace
    xyz(records)                                            float32 [n][3] of 16-byte records
    candidates / votes(sp, records, n, labels)              PLANE_DTYPE [hypotheses]
    best(planes)                                            PLANE_DTYPE record
    inliers(sp, records, n, labels, plane)                  bool [n]
    sums(sp, records, n, labels, plane)                     int64 [10]
    label(sp, records, n, plane, value, labels)             the labels after the call (a copy)
    solve(sp, sums, plane)                                  (plane, dict(inliers, rms, status))
    fit(sp, records, n, labels)                             (plane, stats, trace_sums [iterations][10], trace_planes [iterations + 1])
"""
import math
import types

import numpy as np

PLANE_DTYPE = np.dtype([("normal", np.float32, (3,)), ("offset", np.float32), ("anchor", np.float32, (3,)), ("votes", np.uint32)])
RECORD_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("tag", np.uint32)])
f32 = np.float32
M32 = 0xFFFFFFFF


def spec(hypotheses, dist, span, seed=0, axis=(0.0, 0.0, 0.0), min_cos=0.0, iterations=1, min_inliers=3, min_pivot=0.0):
    return types.SimpleNamespace(hypotheses=int(hypotheses), seed=int(seed) & M32, dist=f32(dist), axis=tuple(f32(a) for a in axis),
                                 min_cos=f32(min_cos), span=f32(span), iterations=int(iterations), min_inliers=int(min_inliers),
                                 min_pivot=f32(min_pivot))


def records_of(points, tags=None):
    """16-byte records from float32 [n][3] (the tag: the index, or `tags`)"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros(len(points), RECORD_DTYPE)
    out["x"], out["y"], out["z"] = points[:, 0], points[:, 1], points[:, 2]
    out["tag"] = np.arange(len(points), dtype=np.uint32) if tags is None else tags
    return out


def xyz(records):
    return np.ascontiguousarray(records).view(np.float32).reshape(-1, 4)[:, :3]


def void_plane():
    return np.zeros(1, PLANE_DTYPE)[0]


def is_void(plane):
    return not np.any(np.asarray(plane["normal"], np.float32) != 0)                  # -0.0 == 0.0: either sign of zero


def mix(seed, k, j):
    """h(seed, k, j) of the header"""
    x = (seed ^ ((k * 0x9E3779B9) & M32)) ^ (((j + 1) * 0x85EBCA6B) & M32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def takes_part(records, n, labels):
    p = xyz(records)[:n]
    ok = np.isfinite(p).all(axis=1)
    if labels is not None:
        ok &= np.asarray(labels)[:n] == 0
    return ok


def threshold(sp):
    a = sp.axis
    with np.errstate(all="ignore"):
        return f32(sp.min_cos * np.sqrt(f32(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2]))))


def has_prior(sp):
    return any(a != 0 for a in sp.axis)


def candidate(sp, records, n, labels, k):
    out = void_plane()
    at = [(mix(sp.seed, k, j) * n) >> 32 for j in range(3)]
    if len(set(at)) < 3:
        return out
    p = xyz(records)
    P = [p[i] for i in at]
    for i, Pi in zip(at, P):
        if not np.isfinite(Pi).all() or (labels is not None and labels[i] != 0):
            return out
    with np.errstate(all="ignore"):
        u, v = P[1] - P[0], P[2] - P[0]
        c = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], np.float32)
        len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if not np.isfinite(len2) or not len2 > 0:
            return out
        nrm = c / np.sqrt(len2)
        if not np.isfinite(nrm).all() or not np.any(nrm != 0):
            return out
        t = (nrm[0] * P[0][0] + nrm[1] * P[0][1]) + nrm[2] * P[0][2]
        if not np.isfinite(t):
            return out
        if has_prior(sp):
            d = (nrm[0] * sp.axis[0] + nrm[1] * sp.axis[1]) + nrm[2] * sp.axis[2]
            if not np.isfinite(d):
                return out
            if d < 0:
                nrm, t, d = -nrm, -t, -d
            if not d >= threshold(sp):
                return out
        elif t > 0:
            nrm, t = -nrm, -t
        out["normal"], out["offset"], out["anchor"], out["votes"] = nrm, f32(0.0) - t, P[0], 0
    return out


def candidates(sp, records, n, labels=None):
    return np.array([candidate(sp, records, n, labels, k) for k in range(sp.hypotheses)], PLANE_DTYPE)


def inliers(sp, records, n, labels, plane):
    ok = takes_part(records, n, labels)
    if is_void(plane):
        return np.zeros(n, bool)
    p = xyz(records)[:n]
    nrm, a = np.asarray(plane["normal"], np.float32), np.asarray(plane["anchor"], np.float32)
    with np.errstate(all="ignore"):
        s = (nrm[0] * (p[:, 0] - a[0]) + nrm[1] * (p[:, 1] - a[1])) + nrm[2] * (p[:, 2] - a[2])
        return ok & np.isfinite(s) & (np.abs(s) <= sp.dist)


def votes(sp, records, n, labels=None):
    planes = candidates(sp, records, n, labels)
    for k in range(sp.hypotheses):
        if not is_void(planes[k]):
            planes["votes"][k] = int(inliers(sp, records, n, labels, planes[k]).sum()) & M32
    return planes


def best(planes):
    pick = None
    for k in range(len(planes)):
        if not is_void(planes[k]) and (pick is None or planes["votes"][k] > planes["votes"][pick]):
            pick = k
    return void_plane() if pick is None else planes[pick].copy()


def quantised(sp, records, n, labels, plane):
    """int64 [m][3]: q of the inliers that are not skipped"""
    mask = inliers(sp, records, n, labels, plane)
    p = xyz(records)[:n][mask]
    a = np.asarray(plane["anchor"], np.float32)
    with np.errstate(all="ignore"):
        e = (p - a[None, :]) / sp.span
        keep = (np.isfinite(e) & (np.abs(e) <= f32(8.0))).all(axis=1)
        return np.rint(e[keep] * f32(65536.0)).astype(np.int64)


def sums(sp, records, n, labels, plane):
    q = quantised(sp, records, n, labels, plane)
    q4 = np.concatenate([q, np.ones((len(q), 1), np.int64)], axis=1)
    return np.array([int((q4[:, i] * q4[:, j]).sum()) for i in range(4) for j in range(i, 4)], np.int64)


def label(sp, records, n, plane, value, labels):
    out = np.array(labels, np.uint8)
    out[:n][inliers(sp, records, n, out, plane)] = value
    return out


def _dot(p, r):
    return (p[0] * r[0] + p[1] * r[1]) + p[2] * r[2]


def _cross(p, r):
    return [p[1] * r[2] - p[2] * r[1], p[2] * r[0] - p[0] * r[2], p[0] * r[1] - p[1] * r[0]]


def _to_f32(v):
    with np.errstate(all="ignore"):
        return f32(v)


def solve(sp, sums10, plane):
    """sgm_plane_solve.  Python floats are IEEE doubles and every line below is one rounding per operation, as the C is."""
    S = [int(v) for v in sums10]
    count = S[9]
    out = np.array(plane, PLANE_DTYPE).copy()
    stats = dict(inliers=count & M32, rms=0.0, status=0)
    if count < sp.min_inliers:
        stats["status"] = 1
        return out, stats
    n = [float(v) for v in plane["normal"]]
    A = [float(v) for v in plane["anchor"]]
    N = float(count)
    M = [[float(S[0]), float(S[1]), float(S[2])], [float(S[1]), float(S[4]), float(S[5])], [float(S[2]), float(S[5]), float(S[7])]]
    m = [float(S[3]), float(S[6]), float(S[8])]
    ln = math.sqrt(_dot(n, n))
    w = [n[0] / ln, n[1] / ln, n[2] / ln]
    axis = 0
    for i in (1, 2):
        if abs(w[i]) < abs(w[axis]):
            axis = i
    e = [0.0, 0.0, 0.0]
    e[axis] = 1.0
    c = _cross(w, e)
    lc = math.sqrt(_dot(c, c))
    t1 = [c[0] / lc, c[1] / lc, c[2] / lc]
    t2 = _cross(w, t1)
    moment = lambda p, r: _dot(p, [_dot(M[0], r), _dot(M[1], r), _dot(M[2], r)])
    Su, Sv, Ss = _dot(t1, m), _dot(t2, m), _dot(w, m)
    Suu, Suv, Svv = moment(t1, t1), moment(t1, t2), moment(t2, t2)
    Sus, Svs, Sss = moment(t1, w), moment(t2, w), moment(w, w)
    Am = [[N, Su, Sv], [Su, Suu, Suv], [Sv, Suv, Svv]]
    y = [Ss, Sus, Svs]
    L = [[0.0] * 3 for _ in range(3)]
    D, z, x = [0.0] * 3, [0.0] * 3, [0.0] * 3
    pivot = float(sp.min_pivot)
    for j in range(3):
        acc = 0.0
        for k in range(j):
            acc += (L[j][k] * L[j][k]) * D[k]
        D[j] = Am[j][j] - acc
        if not math.isfinite(D[j]) or not D[j] > pivot * Am[j][j]:
            stats["status"] = 2
            return out, stats
        for i in range(j + 1, 3):
            acc = 0.0
            for k in range(j):
                acc += (L[i][k] * L[j][k]) * D[k]
            L[i][j] = (Am[i][j] - acc) / D[j]
    for i in range(3):
        acc = 0.0
        for k in range(i):
            acc += L[i][k] * z[k]
        z[i] = y[i] - acc
    for i in (2, 1, 0):
        acc = 0.0
        for k in range(i + 1, 3):
            acc += L[k][i] * x[k]
        x[i] = z[i] / D[i] - acc
    if not all(math.isfinite(v) for v in x):
        stats["status"] = 2
        return out, stats
    g = [(w[i] - x[1] * t1[i]) - x[2] * t2[i] for i in range(3)]
    lg = math.sqrt(_dot(g, g))
    if not math.isfinite(lg) or not lg > 0.0:
        stats["status"] = 2
        return out, stats
    nn = [g[0] / lg, g[1] / lg, g[2] / lg]
    gq = [m[0] / N, m[1] / N, m[2] / N]
    d = x[0] / lg - _dot(nn, gq)
    unit = float(sp.span) / 65536.0
    anchor = [_to_f32(A[i] + (gq[i] + d * nn[i]) * unit) for i in range(3)]
    normal = [_to_f32(nn[i]) for i in range(3)]
    Nf, af = [float(v) for v in normal], [float(v) for v in anchor]
    t = _dot(Nf, af)
    flip = _dot(Nf, [float(a) for a in sp.axis]) < 0.0 if has_prior(sp) else t > 0.0
    if flip:
        normal, t = [-v for v in normal], -t
    offset = _to_f32(0.0 - t)
    ssr = Sss - ((x[0] * Ss + x[1] * Sus) + x[2] * Svs)
    if not ssr >= 0.0:
        ssr = 0.0
    rms = unit * math.sqrt(ssr / N)
    if not (math.isfinite(offset) and math.isfinite(rms) and all(math.isfinite(v) for v in normal + anchor) and any(v != 0 for v in normal)):
        stats["status"] = 2
        return out, stats
    out["normal"], out["offset"], out["anchor"], out["votes"] = normal, offset, anchor, count & M32
    stats["rms"] = rms
    return out, stats


def fit(sp, records, n, labels=None):
    trace_sums = np.zeros((sp.iterations, 10), np.int64)
    trace_planes = np.zeros(sp.iterations + 1, PLANE_DTYPE)
    cur = best(votes(sp, records, n, labels))
    trace_planes[0] = cur
    stats = dict(inliers=0, rms=0.0, status=0)
    if is_void(cur):
        stats["status"] = 1
        return cur, stats, trace_sums, trace_planes
    for it in range(sp.iterations):
        trace_sums[it] = sums(sp, records, n, labels, cur)
        cur, stats = solve(sp, trace_sums[it], cur)
        trace_planes[it + 1] = cur
        if stats["status"] != 0:
            break
    return cur, stats, trace_sums, trace_planes
