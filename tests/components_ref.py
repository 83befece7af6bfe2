"""Restatement of the components section of include/sgm_mi355x.h (sgm_volume_components, sgm_volume_component_of,
sgm_component_metric) in numpy: the set with its plane exclusion in float32, the components by repeated minimum over neighbours to a
fixed point (not the kernels' route: no tiles, no runs, no union-find), the records, and the lookup of a list's objects.  Arrays are
[nz][ny][nx], as the volume.

    member(words, v, min_weight, set, unknown, planes, clearance)   -> bool: the set of a call
    roots(member, connectivity)                                     -> int64: per voxel the smallest voxel index of its component, -1 outside
    components(member, connectivity, min_voxels)                    -> (labels uint32, objects COMPONENT, (C, all))
    call(words, v, ...)                                             -> components(member(...), ...)
    component_of(labels, objects, written, ids, id_kinds)           -> uint32: what sgm_volume_component_of writes
    metric(v, obj)                                                  -> (lo, hi, centroid) float32 [3] each
"""
import itertools

import numpy as np

COMPONENT = np.dtype([("first", np.uint32), ("voxels", np.uint32), ("lo", np.uint16, (3,)), ("hi", np.uint16, (3,)),
                      ("reserved", np.uint32), ("sum", np.uint64, (3,))])
assert COMPONENT.itemsize == 48
# the far corner of edge kind e (the mesh contract's table; kinds 0..2 are the axes of the surface list)
EDGE_STEP = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
_NONE = np.int64(1) << 40


def observed_negative(words, min_weight):
    words = np.asarray(words, np.uint32)
    observed = (words >> 16) >= np.uint32(min_weight)
    tq = (words & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16)
    return observed, tq < 0


def excluded(v, normal, anchor, clearance):
    """bool [nz][ny][nx]: the voxels one plane excludes; float32, every operation rounded on its own"""
    f = np.float32
    n, a = np.asarray(normal, f), np.asarray(anchor, f)
    if not np.any(n != 0):                                       # a void plane (either sign of zero)
        return np.zeros((v.nz, v.ny, v.nx), bool)
    cx, cy, cz = (f(o) + (np.arange(m, dtype=f) + f(0.5)) * f(v.voxel) for o, m in zip(v.origin, (v.nx, v.ny, v.nz)))
    with np.errstate(all="ignore"):
        tx = (n[0] * (cx - a[0]))[None, None, :]
        ty = (n[1] * (cy - a[1]))[None, :, None]
        tz = (n[2] * (cz - a[2]))[:, None, None]
        s = ((tx + ty).astype(f) + tz).astype(f)
        return np.isfinite(s) & (s <= f(clearance))


def member(words, v, min_weight, set=0, unknown=0, planes=(), clearance=()):
    """planes: records with `normal` and `anchor` (PLANE_DTYPE of the package, or tuples (normal, anchor))"""
    observed, neg = observed_negative(np.asarray(words).reshape(v.nz, v.ny, v.nx), min_weight)
    m = (observed & (~neg if set else neg)) | (bool(unknown) & ~observed)
    assert len(planes) == len(clearance) <= 4
    for pl, c in zip(planes, clearance):
        normal, anchor = (pl["normal"], pl["anchor"]) if isinstance(pl, (np.void, np.ndarray)) else pl
        m = m & ~excluded(v, normal, anchor, c)
    return m


def offsets(connectivity):
    assert connectivity in (6, 26)
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0) and (connectivity == 26 or sum(map(abs, d)) == 1)]


def roots(member, connectivity):
    member = np.asarray(member, bool)
    nz, ny, nx = member.shape
    index = np.arange(member.size, dtype=np.int64).reshape(member.shape)
    lab = np.where(member, index, _NONE)
    steps = offsets(connectivity)
    while True:
        new = lab.copy()
        for dz, dy, dx in steps:
            src = tuple(slice(max(d, 0), n + min(d, 0)) for d, n in zip((dz, dy, dx), (nz, ny, nx)))
            dst = tuple(slice(max(-d, 0), n + min(-d, 0)) for d, n in zip((dz, dy, dx), (nz, ny, nx)))
            np.minimum(new[dst], lab[src], out=new[dst])
        new = np.where(member, new, _NONE)
        # (a label is the index of a voxel of the same component: its label is one as well, and no larger)
        flat = new.reshape(-1)
        inside = flat != _NONE
        flat[inside] = flat[flat[inside]]
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(member, lab, -1)


def components(member, connectivity, min_voxels=1):
    member = np.asarray(member, bool)
    nz, ny, nx = member.shape
    root = roots(member, connectivity).reshape(-1)
    inside = root >= 0
    firsts, inverse, sizes = np.unique(root[inside], return_inverse=True, return_counts=True)
    keep = sizes >= min_voxels
    labels = np.zeros(member.size, np.uint32)
    labels[inside] = np.where(keep[inverse], firsts[inverse] + 1, 0)
    objects = np.zeros(int(keep.sum()), COMPONENT)
    n = np.nonzero(inside)[0]
    coords = (n % nx, n // nx % ny, n // (nx * ny))
    rank = np.cumsum(keep) - 1
    objects["first"], objects["voxels"] = firsts[keep], sizes[keep]
    sel = keep[inverse]
    at = rank[inverse[sel]]
    for a, c in enumerate(coords):
        lo = np.full(len(objects), 0xFFFF, np.int64)
        hi = np.zeros(len(objects), np.int64)
        total = np.zeros(len(objects), np.uint64)
        np.minimum.at(lo, at, c[sel])
        np.maximum.at(hi, at, c[sel])
        np.add.at(total, at, c[sel].astype(np.uint64))
        objects["lo"][:, a], objects["hi"][:, a], objects["sum"][:, a] = lo, hi, total
    return labels.reshape(member.shape), objects, (int(keep.sum()), int(len(firsts)))


def call(words, v, min_weight, set=0, unknown=0, connectivity=6, min_voxels=1, planes=(), clearance=()):
    return components(member(words, v, min_weight, set, unknown, planes, clearance), connectivity, min_voxels)


def component_of(labels, objects, written, ids, id_kinds):
    """written: min(C, capacity), the records of `objects` that exist on the device"""
    assert id_kinds in (4, 8)
    labels = np.asarray(labels, np.uint32)
    nz, ny, nx = labels.shape
    flat = labels.reshape(-1)
    firsts = np.asarray(objects["first"][:written], np.int64)
    out = np.zeros(len(ids), np.uint32)
    for r, word in enumerate(np.asarray(ids, np.uint32).astype(np.int64)):
        n, e = divmod(int(word), id_kinds)
        if n >= flat.size or e >= id_kinds - 1:
            continue
        label = int(flat[n])
        if label == 0:
            i, j, k = n % nx + EDGE_STEP[e][0], n // nx % ny + EDGE_STEP[e][1], n // (nx * ny) + EDGE_STEP[e][2]
            if i < nx and j < ny and k < nz:
                label = int(labels[k, j, i])
        if label:
            hit = np.nonzero(firsts == label - 1)[0]
            if len(hit):
                out[r] = hit[0] + 1
    return out


def metric(v, obj):
    f = np.float32
    origin = np.asarray(v.origin, f)
    lo = origin + obj["lo"].astype(f) * f(v.voxel)
    hi = origin + (obj["hi"].astype(np.int64) + 1).astype(f) * f(v.voxel)
    mean = obj["sum"].astype(np.float64) / np.float64(obj["voxels"]) if obj["voxels"] else np.zeros(3)
    centroid = (origin.astype(np.float64) + (mean + 0.5) * np.float64(f(v.voxel))).astype(f)
    return lo.astype(f), hi.astype(f), centroid
