#!/usr/bin/env python3
"""The (tetrahedron, sign mask) -> triangles table of csrc/sgm_mesh.hip (MESH_TABLE), generated from the contract of
include/sgm_mi355x.h (sgm_volume_mesh): the edges of each triangle in the contract's order, wound by the midpoint rule.

    python tools/mesh_table.py            prints the table as the rows of the constexpr array
    table()                               -> [6][16][2] words (tests/test_mesh_cpu.py compares them with tests/mesh_ref.py, which
                                             computes the rule geometrically, and with the array in the source)

A word holds one triangle, three 6-bit vertex codes (v0 in the low bits): code = corner | kind << 3, the edge of kind `kind`
(0..6: steps (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)) that starts at corner `corner` = dx | dy << 1 | dz << 2 of
the cell.  Masks 0 and 15 and the second word of a mask with one or three negative corners are 0: the kernels take the number of
triangles from the mask's population count.  Integers only: midpoints are doubled, centroids are scaled by the set sizes."""
import itertools

PERMS = list(itertools.permutations(range(3)))              # (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x)
KIND = {(1, 0, 0): 0, (0, 1, 0): 1, (0, 0, 1): 2, (1, 1, 0): 3, (1, 0, 1): 4, (0, 1, 1): 5, (1, 1, 1): 6}


def corners(t):
    """the four corners of tetrahedron t, a path from (0,0,0) to (1,1,1) along the axes of PERMS[t]"""
    out = [(0, 0, 0)]
    for axis in PERMS[t]:
        out.append(tuple(1 if d == axis else c for d, c in enumerate(out[-1])))
    return out


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def triangles(t, mask):
    """the wound triangles of (t, mask), each three edges (a, b) with a < b, indices into corners(t)"""
    N = [i for i in range(4) if mask >> i & 1]
    P = [i for i in range(4) if not mask >> i & 1]
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(N) in (0, 4):
        return []
    if len(N) == 1:
        tris = [[edge(N[0], p) for p in P]]
    elif len(N) == 3:
        tris = [[edge(P[0], n) for n in N]]
    else:
        (a, b), (c, d) = N, P
        tris = [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
    p = corners(t)
    total = lambda idx: tuple(sum(p[i][d] for i in idx) for d in range(3))
    away = tuple(len(N) * cp - len(P) * cn for cp, cn in zip(total(P), total(N)))      # |N||P| (centroid(P) - centroid(N))
    out = []
    for tri in tris:
        m = [tuple(p[a][d] + p[b][d] for d in range(3)) for a, b in tri]              # twice the midpoints
        n = cross(tuple(m[1][d] - m[0][d] for d in range(3)), tuple(m[2][d] - m[0][d] for d in range(3)))
        s = sum(n[d] * away[d] for d in range(3))
        assert s != 0, (t, mask)
        out.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return out


def code(t, a, b):
    p = corners(t)
    lo, hi = p[a], p[b]
    return (lo[0] | lo[1] << 1 | lo[2] << 2) | KIND[tuple(h - l for h, l in zip(hi, lo))] << 3


def table():
    out = []
    for t in range(6):
        rows = []
        for mask in range(16):
            words = [sum(code(t, a, b) << (6 * k) for k, (a, b) in enumerate(tri)) for tri in triangles(t, mask)]
            rows.append((words + [0, 0])[:2])
        out.append(rows)
    return out


def rows():
    """the lines between the braces of MESH_TABLE"""
    return ["    {" + ", ".join("{0x%05x, 0x%05x}" % tuple(w) for w in row) + "}," for row in table()]


if __name__ == "__main__":
    print("\n".join(rows()))
