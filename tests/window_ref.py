"""Restatement of the window section of include/sgm_mi355x.h (sgm_volume_window, sgm_volume_follow, sgm_volume_leaving) in numpy:
words are copied, the window's origin is float32 arithmetic (one product, one sum), the shift is double arithmetic, the boxes are
integers.  Specs are the plain records of volume_ref.spec.

    window_spec(src, offset, dims)          -> the window's spec, None where the call refuses
    window(words, src, offset, dims)        -> uint32 [dims[2]][dims[1]][dims[0]]: the window of one array of words
    follow(v, pose, focus_z, granule, margin) -> (sx, sy, sz), None where the call refuses
    ranges(v, shift)                        -> per axis ((leave begin, end), (stay begin, end)) in cells
    leaving(v, shift)                       -> [(lo, n), ...]: the boxes that leave, in voxels, at most three
    stay_box(v, shift)                      -> (lo, n) of the cells that stay, None where there are none
"""
import math

import numpy as np

import volume_ref as VR

MAX_OFFSET = 1 << 20


def _spec_ok(v):
    f = np.float32
    return (all(1 <= n <= 1024 for n in (v.nx, v.ny, v.nz)) and v.nx * v.ny * v.nz <= 1 << 30 and 1 <= v.max_weight <= 65535 and
            all(np.isfinite(f(x)) and f(x) > 0 for x in (v.voxel, v.trunc)) and all(np.isfinite(f(o)) for o in v.origin))


def window_spec(src, offset, dims):
    f = np.float32
    if not _spec_ok(src) or any(abs(int(o)) > MAX_OFFSET for o in offset):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        origin = [f(f(o) + f(f(int(d)) * f(src.voxel))) for o, d in zip(src.origin, offset)]      # the product, then the sum
    out = VR.spec(int(dims[0]), int(dims[1]), int(dims[2]), src.voxel, origin, src.trunc, src.max_weight)
    return out if _spec_ok(out) else None


def window(words, src, offset, dims):
    """destination (i, j, k) = source (i + ox, j + oy, k + oz) where that is inside the source grid, else 0"""
    words = np.asarray(words, np.uint32).reshape(src.nz, src.ny, src.nx)
    out = np.zeros((dims[2], dims[1], dims[0]), np.uint32)
    cut = []
    for n_src, n_dst, o in zip((src.nx, src.ny, src.nz), dims, offset):
        lo, hi = max(0, -o), min(n_dst, n_src - o)                # the destination indices whose source index is inside
        if hi <= lo:
            return out
        cut.append((slice(lo, hi), slice(lo + o, hi + o)))
    (dx, sx), (dy, sy), (dz, sz) = cut
    out[dz, dy, dx] = words[sz, sy, sx]
    return out


def follow(v, pose, focus_z, granule, margin):
    """in double (Python floats), every operation on its own, sums left to right"""
    p = [float(x) for x in np.asarray(pose, np.float32).reshape(12)]
    fz = float(np.float32(focus_z))
    if not _spec_ok(v) or granule < 1 or margin < 0 or not all(math.isfinite(x) for x in p + [fz]):
        return None
    c = (0.0 - p[9], 0.0 - p[10], fz - p[11])
    out = []
    for a, n in enumerate((v.nx, v.ny, v.nz)):
        P = (p[a] * c[0] + p[3 + a] * c[1]) + p[6 + a] * c[2]
        g = (P - float(np.float32(v.origin[a]))) / float(np.float32(v.voxel)) - n / 2.0
        if not abs(g) < MAX_OFFSET:
            return None
        sh = 0.0 if abs(g) <= margin else granule * math.floor(g / granule + 0.5)
        if abs(sh) > MAX_OFFSET:
            return None
        out.append(int(sh))
    return tuple(out)


def ranges(v, shift):
    out = []
    for n, s in zip((v.nx, v.ny, v.nz), shift):
        c = n - 1
        if s > 0:
            out.append(((0, min(s, c)), (min(s, c), c)))
        elif s < 0:
            out.append(((max(c + s, 0), c), (0, max(c + s, 0))))
        else:
            out.append(((0, 0), (0, c)))
    return out


def _box(parts):
    if any(hi <= lo for lo, hi in parts):
        return None
    return tuple(lo for lo, _ in parts), tuple(hi - lo + 1 for lo, hi in parts)


def leaving(v, shift):
    r = ranges(v, shift)
    cells = [(0, n - 1) for n in (v.nx, v.ny, v.nz)]
    boxes = (_box([r[i][1] if i < a else r[i][0] if i == a else cells[i] for i in range(3)]) for a in range(3))
    return [b for b in boxes if b is not None]


def stay_box(v, shift):
    return _box([r[1] for r in ranges(v, shift)])
