"""Restatement in numpy of the matching at 1/f scale defined in include/sgm_mi355x.h (sgm_scale_spec): the box downscale, the
prior by guided selection and the re-search on the full-resolution census words.  Written from the header's text, vectorised over
the pixels of one frame; tests/test_scaled_cpu.py checks it against a plain double loop of the same text.  Every function takes
one frame ([H][W] arrays) unless it says otherwise."""
import numpy as np

OUTSIDE = 24                       # the cost of a window pixel, or of its partner in the other view, outside the frame
PRIOR_MAX = np.float32(1 << 20)    # priors are clamped to +-2^20 before they are rounded
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.int32)


def popcount32(v):
    v = np.asarray(v, np.uint32)
    return _POP16[v & np.uint32(0xFFFF)] + _POP16[v >> np.uint32(16)]


def finite_bits(a):
    """finite by the bit pattern of a float32 array: the exponent bits are not all ones"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def scaled_shape(width, height, f):
    return width // f, height // f


def downscale(img, f):
    """[..., H, W] u8 / u16 -> [..., H // f, W // f]: (sum of the f x f block + f^2 / 2) >> log2(f^2)"""
    img = np.asarray(img)
    H, W = img.shape[-2:]
    h, w = H // f, W // f
    blocks = img[..., :h * f, :w * f].astype(np.uint32).reshape(img.shape[:-2] + (h, f, w, f))
    return ((blocks.sum(axis=(-3, -1)) + np.uint32(f * f // 2)) >> np.uint32({2: 2, 4: 4}[f])).astype(img.dtype)


def _axis(n_full, n_small, f):
    """per full-resolution coordinate: the two clamped low-resolution indices and the weight numerator a"""
    n = 2 * np.arange(n_full, dtype=np.int64) + 1 - f
    k0 = np.floor_divide(n, 2 * f)
    a = n - 2 * f * k0
    return np.clip(k0, 0, n_small - 1), np.clip(k0 + 1, 0, n_small - 1), a


def prior(disp_small, guide_small, guide_full, f):
    """f * the selected low-resolution disparity per full-resolution pixel, +INF where no candidate is finite"""
    H, W = guide_full.shape
    h, w = disp_small.shape
    j0, j1, ay = _axis(H, h, f)
    i0, i1, ax = _axis(W, w, f)
    g = guide_full.astype(np.int64)
    best = np.full((H, W), np.inf, np.float32)
    best_diff = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    best_w = np.full((H, W), -1, np.int64)
    cands = ((j0, i0, 2 * f - ay, 2 * f - ax), (j0, i1, 2 * f - ay, ax), (j1, i0, ay, 2 * f - ax), (j1, i1, ay, ax))
    for jj, ii, wy, wx in cands:
        d = disp_small[jj[:, None], ii[None, :]]
        diff = np.abs(guide_small[jj[:, None], ii[None, :]].astype(np.int64) - g)
        wgt = wy[:, None] * wx[None, :]
        take = finite_bits(d) & ((diff < best_diff) | ((diff == best_diff) & (wgt > best_w)))
        best = np.where(take, d, best).astype(np.float32)
        best_diff = np.where(take, diff, best_diff)
        best_w = np.where(take, wgt, best_w)
    return np.where(finite_bits(best), np.float32(f) * best, best).astype(np.float32)


def window_costs(census_ref, census_oth, d, radius, right_view):
    """A(d) per pixel for the per-pixel integer disparities d"""
    H, W = census_ref.shape
    ys, xs = np.mgrid[0:H, 0:W]
    A = np.zeros((H, W), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qy, qx = ys + dy, xs + dx
            xo = qx + d if right_view else qx - d
            ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W) & (xo >= 0) & (xo < W)
            cy, cx, co = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1), np.clip(xo, 0, W - 1)
            A += np.where(ok, popcount32(census_ref[cy, cx] ^ census_oth[cy, co]), OUTSIDE)
    return A


def upscale(disp_small, guide_small, guide_full, census_ref, census_oth, f, radius, penalty, d_lo, d_hi, right_view):
    """sgm_upscale_disparity on one frame"""
    pr = prior(np.ascontiguousarray(disp_small, np.float32), guide_small, guide_full, f)
    if radius < 0:
        return pr
    fin = finite_bits(pr)
    p = np.rint(np.clip(np.where(fin, pr, np.float32(0)), -PRIOR_MAX, PRIOR_MAX)).astype(np.int64)
    win = (2 * radius + 1) ** 2
    offs = list(range(-f, f + 1))
    C = np.stack([2 * window_costs(census_ref, census_oth, p + o, radius, right_view) + penalty * abs(o) * win for o in offs])
    adm = np.stack([(p + o >= d_lo) & (p + o <= d_hi) for o in offs])
    # smallest C, then smaller |o|, then smaller d: candidates in the order 0, -1, +1, ... with a strict compare
    best = np.full(p.shape, -1, np.int64)
    bc = np.full(p.shape, np.iinfo(np.int64).max, np.int64)
    for o in sorted(offs, key=lambda o: (abs(o), o)):
        k = o + f
        take = adm[k] & (C[k] < bc)
        best = np.where(take, k, best)
        bc = np.where(take, C[k], bc)
    any_adm = best >= 0
    kb = np.clip(best, 0, 2 * f)
    km, kp = np.clip(kb - 1, 0, 2 * f), np.clip(kb + 1, 0, 2 * f)
    take = lambda a, k: np.take_along_axis(a, k[None], 0)[0]
    cm, cp = take(C, km), take(C, kp)
    both = (kb >= 1) & (kb <= 2 * f - 1) & take(adm, km) & take(adm, kp)
    den = cm + cp - 2 * bc
    sub = both & (den > 0) & any_adm
    d = (p + kb - f).astype(np.float32)
    with np.errstate(all="ignore"):
        frac = (cm - cp).astype(np.float32) / np.where(sub, 2 * den, 1).astype(np.float32)
    out = np.where(sub, d + frac, d).astype(np.float32)
    return np.where(fin & any_adm, out, pr).astype(np.float32)


def upscale_batch(disp_small, guide_small, guide_full, census_ref, census_oth, f, radius, penalty, d_lo, d_hi, right_view):
    """the same on [frames][..][..] stacks (census planes may be None with radius < 0)"""
    n = len(disp_small)
    cr = census_ref if census_ref is not None else [None] * n
    co = census_oth if census_oth is not None else [None] * n
    return np.stack([upscale(disp_small[i], guide_small[i], guide_full[i], cr[i], co[i], f, radius, penalty, d_lo, d_hi, right_view)
                     for i in range(n)])


def nearest_upscale(disp_small, f, H, W):
    """the plain upscale a caller gets today: f * the low-resolution pixel under the full-resolution one"""
    h, w = disp_small.shape
    jj = np.minimum(np.arange(H) // f, h - 1)
    ii = np.minimum(np.arange(W) // f, w - 1)
    return (np.float32(f) * disp_small[jj[:, None], ii[None, :]]).astype(np.float32)


def bad_share(disp, gt, thresh=1.0):
    """share of the pixels with known ground truth that are invalid or off by more than thresh"""
    known = np.isfinite(gt) & (gt > 0)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(disp) | (np.abs(disp - gt) > thresh)
    return float((bad & known).sum()) / float(known.sum())
