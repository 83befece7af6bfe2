"""Restatement of the distance section of include/sgm_mi355x.h (sgm_volume_distance, sgm_volume_distance_field) in numpy: the site
predicate, the windowed separable transform in exact integers, and the float32 field.  Arrays are [nz][ny][nx], as the volume.

    sites(words, min_weight, side, unknown)          -> bool: the sites of a call
    transform(site, r)                               -> uint16: squared distance to the nearest site, FAR beyond r
    distance(words, min_weight, r, side, unknown)    -> uint16: what sgm_volume_distance writes
    field(o, i, voxel)                               -> float32: what sgm_volume_distance_field writes (i may be None)
"""
import numpy as np

FAR = 0xFFFF
_BIG = 1 << 40


def obstacles(words, min_weight, unknown):
    """bool: the obstacle set O -- observed (w >= min_weight) with tq < 0, and the unobserved voxels where unknown == 1"""
    words = np.asarray(words, np.uint32)
    observed = (words >> 16) >= np.uint32(min_weight)
    tq = (words & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16)
    return (observed & (tq < 0)) | (bool(unknown) & ~observed)


def sites(words, min_weight, side, unknown):
    o = obstacles(words, min_weight, unknown)
    return ~o if side else o


def _pass(g, axis, r):
    """out[j] = min over |o| <= r of g[j + o] + o * o along `axis`, nothing outside the grid; values above r * r pruned at once"""
    n = g.shape[axis]
    out = g.copy()                                                # o == 0
    for o in range(1, min(r, n - 1) + 1):
        for sign in (1, -1):
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            if sign > 0:
                src[axis], dst[axis] = slice(o, n), slice(0, n - o)
            else:
                src[axis], dst[axis] = slice(0, n - o), slice(o, n)
            np.minimum(out[tuple(dst)], g[tuple(src)] + o * o, out=out[tuple(dst)])
    out[out > r * r] = _BIG
    return out


def transform(site, r):
    site = np.asarray(site, bool)
    assert site.ndim == 3 and 1 <= r <= 255
    g = np.where(site, 0, _BIG).astype(np.int64)
    for axis in (2, 1, 0):                                        # x, then y, then z
        g = _pass(g, axis, r)
    return np.where(g <= r * r, g, FAR).astype(np.uint16)


def distance(words, min_weight, r, side=0, unknown=0):
    return transform(sites(words, min_weight, side, unknown), r)


def field(o, i, voxel):
    """float32, every operation rounded on its own"""
    f = np.float32
    o = np.asarray(o, np.uint16)
    with np.errstate(invalid="ignore"):
        pos = f(voxel) * np.sqrt(o.astype(np.float32))
    out = np.where(o == FAR, f(np.inf), pos).astype(np.float32)
    if i is None:
        return out                                                # o == 0 gives voxel * 0 = 0
    i = np.asarray(i, np.uint16)
    neg = -(f(voxel) * np.sqrt(i.astype(np.float32)))
    inside = np.where(i == 0, f(0.0), np.where(i == FAR, f(-np.inf), neg)).astype(np.float32)
    return np.where(o == 0, inside, out).astype(np.float32)
