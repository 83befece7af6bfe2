"""Restatement of the mesh contract of include/sgm_mi355x.h (sgm_volume_mesh), numpy on float32 arrays: marching tetrahedra over a
volume as sgm_volume_integrate leaves it.  Every float operation is one IEEE float32 operation, as in the kernels.  The triangles of
a (tetrahedron, sign mask) and their winding are computed here from the geometry -- midpoints and centroids as the contract words
them -- not read from the table the kernels carry.

    tet_corners(t)                      -> the four corners of tetrahedron t in the unit cell, [4][3] ints
    case_triangles(t, mask)             -> the wound triangles of a case: a list of three edges (a, b), a < b, corner indices
    case_codes(t, mask)                 -> the same as two words of 6-bit vertex codes, the layout of MESH_TABLE in csrc/sgm_mesh.hip
    vertices(vox, v, min_weight)        -> VERTEX records sorted by id
    mesh(vox, v, min_weight)            -> (VERTEX records, TRIANGLE records)
    closed(tri)                         -> every directed edge occurs exactly once and its reverse exactly once
    euler(tri)                          -> V - E + F over the vertices the triangles use
    signed_volume(vert, tri)            -> float64: positive when the normals point out of the enclosed solid
    sphere(dims, zero_below=0)          -> a planted volume: a sphere of negative tq in a positive field, all weights 1
"""
import functools
import itertools

import numpy as np

import volume_ref as VR

VERTEX = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("id", np.uint32)])
TRIANGLE = np.dtype([("v", np.uint32, (3,)), ("cell", np.uint32)])
KINDS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]         # (dx, dy, dz) of edge kind e
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]                   # (a, b, c) of tetrahedron t
MAX_VOXELS = 1 << 27


def tet_corners(t):
    p = np.zeros((4, 3), np.int64)
    for step, axis in enumerate(PERMS[t]):
        p[step + 1] = p[step]
        p[step + 1, axis] = 1
    return p


@functools.lru_cache(maxsize=None)
def case_triangles(t, mask):
    N = [i for i in range(4) if mask >> i & 1]
    P = [i for i in range(4) if not mask >> i & 1]
    e = lambda a, b: (min(a, b), max(a, b))
    if len(N) in (0, 4):
        return ()
    if len(N) == 1:
        tris = [[e(N[0], P[0]), e(N[0], P[1]), e(N[0], P[2])]]
    elif len(N) == 3:
        tris = [[e(P[0], N[0]), e(P[0], N[1]), e(P[0], N[2])]]
    else:
        (a, b), (c, d) = N, P
        tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    p = tet_corners(t).astype(np.float64)
    away = p[P].mean(axis=0) - p[N].mean(axis=0)                   # centroid(P) - centroid(N)
    out = []
    for tri in tris:
        m = [(p[a] + p[b]) / 2 for a, b in tri]                   # each vertex at the midpoint of its edge
        s = float(np.cross(m[1] - m[0], m[2] - m[0]) @ away)
        assert abs(s) > 1e-9, (t, mask)
        out.append(tuple(tri) if s > 0 else (tri[0], tri[2], tri[1]))
    return tuple(out)


def edge_code(t, a, b):
    """(corner of the cell, kind) of the edge between corners a < b of tetrahedron t: taken from its lower corner"""
    p = tet_corners(t)
    lo, d = p[a], tuple(int(x) for x in p[b] - p[a])
    return int(lo[0] | lo[1] << 1 | lo[2] << 2), KINDS.index(d)


def case_codes(t, mask):
    words = []
    for tri in case_triangles(t, mask):
        word = 0
        for k, (a, b) in enumerate(tri):
            corner, kind = edge_code(t, a, b)
            word |= (corner | kind << 3) << (6 * k)
        words.append(word)
    return (words + [0, 0])[:2]


def _lo_hi(d):
    """slices of the [nz][ny][nx] arrays for an edge that steps d = (dx, dy, dz): its lower and its far voxels"""
    lo = tuple(slice(0, -1) if d[2 - ax] else slice(None) for ax in range(3))
    hi = tuple(slice(1, None) if d[2 - ax] else slice(None) for ax in range(3))
    return lo, hi


def vertices(vox, v, min_weight):
    f = np.float32
    tq, w = VR.unpack(np.asarray(vox).reshape(v.nz, v.ny, v.nx))
    c = VR.centres(v)
    n = np.arange(v.nx * v.ny * v.nz, dtype=np.int64).reshape(v.nz, v.ny, v.nx)
    recs = []
    for e, d in enumerate(KINDS):
        lo, hi = _lo_hi(d)
        cross = (w[lo] >= min_weight) & (w[hi] >= min_weight) & ((tq[lo] < 0) != (tq[hi] < 0))
        k, j, i = np.nonzero(cross)
        tn, tm = tq[lo][cross].astype(f), tq[hi][cross].astype(f)
        with np.errstate(all="ignore"):
            s = tn / (tn - tm)
        step = s * f(v.voxel)
        assert step.dtype == np.float32
        rec = np.empty(i.size, VERTEX)
        rec["x"], rec["y"], rec["z"] = c[0][i], c[1][j], c[2][k]
        for axis, name in enumerate("xyz"):
            if d[axis]:
                rec[name] = rec[name] + step
        rec["id"] = (n[lo][cross] * 8 + e).astype(np.uint32)
        recs.append(rec)
    out = np.concatenate(recs)
    return out[np.argsort(out["id"], kind="stable")]


def triangle_ids(vox, v, min_weight):
    """(ids int64 [T][3], cell int64 [T]) in the contract's order: by cell, then tetrahedron, then first before second"""
    tq, w = VR.unpack(np.asarray(vox).reshape(v.nz, v.ny, v.nx))
    if min(v.nx, v.ny, v.nz) < 2:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    n = np.arange(v.nx * v.ny * v.nz, dtype=np.int64).reshape(v.nz, v.ny, v.nx)
    corner = lambda a, d: a[d[2]:a.shape[0] - 1 + d[2], d[1]:a.shape[1] - 1 + d[1], d[0]:a.shape[2] - 1 + d[0]]
    meshed = np.ones((v.nz - 1, v.ny - 1, v.nx - 1), bool)
    for d in itertools.product((0, 1), repeat=3):
        meshed &= corner(w, d) >= min_weight
    cell = corner(n, (0, 0, 0))
    ids, cells, keys = [], [], []
    for t in range(6):
        p = tet_corners(t)
        mask = sum((corner(tq, tuple(p[i])) < 0).astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            here = meshed & (mask == m)
            if not here.any():
                continue
            for k, tri in enumerate(case_triangles(t, m)):
                rows = []
                for a, b in tri:
                    d = tuple(int(x) for x in p[b] - p[a])
                    rows.append(corner(n, tuple(p[a]))[here] * 8 + KINDS.index(d))
                ids.append(np.stack(rows, axis=1))
                cells.append(cell[here])
                keys.append(cell[here] * 16 + t * 2 + k)
    if not ids:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    ids, cells, keys = np.concatenate(ids), np.concatenate(cells), np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    return ids[order], cells[order]


def mesh(vox, v, min_weight):
    assert v.nx * v.ny * v.nz <= MAX_VOXELS
    vert = vertices(vox, v, min_weight)
    ids, cells = triangle_ids(vox, v, min_weight)
    tri = np.zeros(len(ids), TRIANGLE)
    if len(ids):
        rank = np.searchsorted(vert["id"], ids.reshape(-1))
        assert np.array_equal(vert["id"][rank], ids.reshape(-1))   # every vertex of a triangle is in the list
        tri["v"] = rank.reshape(-1, 3)
        tri["cell"] = cells
    return vert, tri


def _directed(tri):
    v = np.asarray(tri["v"], np.int64)
    return np.concatenate([v[:, [0, 1]], v[:, [1, 2]], v[:, [2, 0]]])


def closed(tri):
    """every directed triangle edge occurs exactly once and its reverse exactly once"""
    if len(tri) == 0:
        return True
    e = _directed(tri)
    big = int(e.max()) + 1
    fwd, back = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(back))


def euler(tri):
    e = np.sort(_directed(tri), axis=1)
    return len(np.unique(tri["v"])) - len(np.unique(e, axis=0)) + len(tri)


def signed_volume(vert, tri):
    p = np.stack([vert["x"], vert["y"], vert["z"]], axis=1).astype(np.float64)
    a, b, c = (p[tri["v"][:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere(dims, zero_below=0):
    """(spec, words): tq the clipped distance to a sphere off the grid's centre, negative inside; |tq| < zero_below planted as 0"""
    nx, ny, nz = dims
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx] + 0.5
    r = np.sqrt((x - nx / 2 - 0.13) ** 2 + (y - ny / 2 + 0.21) ** 2 + (z - nz / 2 - 0.07) ** 2)
    tq = np.rint(np.clip((r - min(dims) / 2 + 1.6) / 2, -1, 1) * 32767).astype(np.int64)
    tq[np.abs(tq) < zero_below] = 0
    v = VR.spec(nx, ny, nz, 0.05, (-0.3, 0.2, 0.9), 0.1)
    return v, VR.pack(tq, np.ones_like(tq))
