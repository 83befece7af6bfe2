"""The centre-symmetric census of include/sgm_mi355x.h (SGM_SetCensusKind) restated in numpy, and the rest of a match chained
from the oracle's own stage functions -- TEST INFRASTRUCTURE ONLY.  Parity unpinned by the reference: the header defines the
census, this module is its checker; everything behind the census words is the oracle's (pinned by the reference).

    census_sym(img, cw, ch)                             u32 [H][W] words
    pipeline(oracle, left, right, opt, cw, ch, ...)     the nine stages of oracle.pyoracle.STAGE_NAMES
    noisy_pair(left, right, sigma)                      the seeded sensor noise of the accuracy table (NOTES.md)
"""
import ctypes as C

import numpy as np

from oracle.pyoracle import STAGE_NAMES

SYMMETRIC_WINDOW = (7, 7)                                  # SGM_CENSUS_SYMMETRIC_DEFAULT_W / _H


def n_bits(cw, ch):
    return (cw * ch - 1) // 2


def census_sym(img, cw, ch):
    """bits = (bits << 1) | (I[y+r][x+c] < I[y-r][x-c]) over the offsets (r, c) strictly before the centre, raster order; 0
    within cw/2 columns or ch/2 rows of the frame edge, and everywhere unless W > cw and H > ch."""
    assert cw >= 1 and ch >= 1 and cw % 2 == 1 and ch % 2 == 1 and cw * ch <= 64
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.uint32)
    if not (w > cw and h > ch):
        return out
    rx, ry = cw // 2, ch // 2
    bits = np.zeros((h - 2 * ry, w - 2 * rx), np.uint32)
    offsets = [(r, c) for r in range(-ry, ry + 1) for c in range(-rx, rx + 1)][:n_bits(cw, ch)]
    for r, c in offsets:
        a = img[ry + r:h - ry + r, rx + c:w - rx + c]
        b = img[ry - r:h - ry - r, rx - c:w - rx - c]
        bits = (bits << np.uint32(1)) | (a < b).astype(np.uint32)
    out[ry:h - ry, rx:w - rx] = bits
    return out


def _lrcheck_right(oracle, dr, dl, thres):
    """the oracle's mirrored LR check (sgmo_lrcheck_right), which oracle.pyoracle.Oracle does not wrap"""
    dr = dr.copy()
    h, w = dr.shape
    f = oracle.lib.sgmo_lrcheck_right
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    f.restype = None
    f(dr.ctypes.data, np.ascontiguousarray(dl).ctypes.data, w, h, thres)
    return dr


def pipeline(oracle, left, right, opt, cw, ch, right_view=False, honor_num_paths=False, words=None, S_prev=None):
    """One match as sgmo_match chains it (oracle/sgm_oracle.c), from symmetric census words: cost -> aggregate_all -> wta x 2
    -> lrcheck -> remove_speckles -> median.  words: (census_l, census_r) to use instead (the pinning test feeds the oracle's
    own 5x5 words).  right_view: the right image's map, checked by the mirrored LR check.  honor_num_paths: num_paths == 4
    runs the first four directions.  S_prev: the aggregated costs of the match before, for a match without Reset (the
    uint16 sums add up and wrap).  Stage 5 is None where the match does not compute the right view."""
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    cl, cr = words if words is not None else (census_sym(left, cw, ch), census_sym(right, cw, ch))
    dmin, dmax = opt.min_disparity, opt.max_disparity
    cost = oracle.cost(np.ascontiguousarray(cl), np.ascontiguousarray(cr), dmin, dmax)
    n_dirs = 4 if (honor_num_paths and opt.num_paths == 4) else 8
    S = oracle.aggregate_all(left, cost, opt.p1, opt.p2_init, n_dirs)
    if S_prev is not None:
        S = (S_prev.astype(np.uint16) + S).astype(np.uint16)
    disp_l = oracle.wta(S, dmin, dmax, bool(opt.is_check_unique), opt.uniqueness_ratio, False)
    disp_r = None
    cur = disp_l
    if opt.is_check_lr or right_view:
        disp_r = oracle.wta(S, dmin, dmax, bool(opt.is_check_unique), opt.uniqueness_ratio, True)
        if right_view:
            cur = _lrcheck_right(oracle, disp_r, disp_l, opt.lrcheck_thres) if opt.is_check_lr else disp_r.copy()
        else:
            cur = oracle.lrcheck(disp_l, disp_r, opt.lrcheck_thres)
    after_lr = cur
    after_speckle = oracle.remove_speckles(after_lr, opt.min_speckle_area) if opt.is_remove_speckles else after_lr.copy()
    final = oracle.median(after_speckle)
    return dict(zip(STAGE_NAMES, (cl, cr, cost, S, disp_l, disp_r, after_lr, after_speckle, final)))


def noisy_pair(left, right, sigma, seed=7):
    """Gaussian sensor noise on both images from ONE generator, the left image first, clipped and rounded to u8."""
    rng = np.random.default_rng(seed)
    out = []
    for img in (left, right):
        out.append(np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, sigma, img.shape)), 0, 255).astype(np.uint8))
    return out[0], out[1]
