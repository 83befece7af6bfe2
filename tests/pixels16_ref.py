"""Restatement of the 16-bit front end of include/sgm_mi355x.h (SGM_SetPixelBits) in numpy -- TEST INFRASTRUCTURE ONLY.  Parity
unpinned by the reference: the header defines the feature, this module is its checker.  Every function takes samples of any
unsigned integer type as they are (no tone map anywhere), so on uint8 input the census functions are the 8-bit formulas, which
tests/test_pixels16_cpu.py pins against the oracle's own census.

    narrow(img, bits)                    u8: g8 = min(v >> (bits - 8), 255)
    census_centre(img, cw, ch)           the centre census: u32 words for 5x5 (the reference's), u64 words for a wide window
    census_sym(img, cw, ch)              the centre-symmetric census: u32 words for any window
    remap_q(img, xq, yq) / remap(...)    the rectification's sampling on samples of any width, same dtype out
    widen(img8, bits)                    u16: v = u8 << (bits - 8), the pair of the shift identity
    rank_pair(left, right)               the dense ranks of a pair with at most 256 distinct values: a u8 pair with the same order
    lut_pair(left8, right8, bits, seed)  v = lut[u8] with a random strictly increasing lut below 2^bits, the pair of the rank identity
"""
import numpy as np

import rectify_ref as RR


def narrow(img, bits):
    assert 9 <= bits <= 16
    return np.minimum(np.asarray(img).astype(np.uint32) >> (bits - 8), 255).astype(np.uint8)


def widen(img8, bits):
    assert 9 <= bits <= 16
    return (np.asarray(img8, np.uint8).astype(np.uint16) << (bits - 8)).astype(np.uint16)


def _window_ok(cw, ch):
    assert cw >= 1 and ch >= 1 and cw % 2 == 1 and ch % 2 == 1 and cw * ch <= 64


def census_centre(img, cw=5, ch=5):
    """bits = (bits << 1) | (I[y+r][x+c] < I[y][x]) over every offset of the window in raster order, the centre included (its
    comparison is 0); 0 within cw/2 columns or ch/2 rows of the frame edge, and everywhere unless W > cw and H > ch."""
    _window_ok(cw, ch)
    img = np.asarray(img)
    h, w = img.shape
    word = np.uint32 if (cw, ch) == (5, 5) else np.uint64
    out = np.zeros((h, w), word)
    if not (w > cw and h > ch):
        return out
    rx, ry = cw // 2, ch // 2
    centre = img[ry:h - ry, rx:w - rx]
    bits = np.zeros(centre.shape, word)
    for r in range(-ry, ry + 1):
        for c in range(-rx, rx + 1):
            bits = (bits << word(1)) | (img[ry + r:h - ry + r, rx + c:w - rx + c] < centre).astype(word)
    out[ry:h - ry, rx:w - rx] = bits
    return out


def census_sym(img, cw, ch):
    """bits = (bits << 1) | (I[y+r][x+c] < I[y-r][x-c]) over the (cw * ch - 1) / 2 offsets strictly before the centre, raster order;
    the same zero border as census_centre."""
    _window_ok(cw, ch)
    img = np.asarray(img)
    h, w = img.shape
    out = np.zeros((h, w), np.uint32)
    if not (w > cw and h > ch):
        return out
    rx, ry = cw // 2, ch // 2
    bits = np.zeros((h - 2 * ry, w - 2 * rx), np.uint32)
    offsets = [(r, c) for r in range(-ry, ry + 1) for c in range(-rx, rx + 1)][:(cw * ch - 1) // 2]
    for r, c in offsets:
        a = img[ry + r:h - ry + r, rx + c:w - rx + c]
        b = img[ry - r:h - ry - r, rx - c:w - rx - c]
        bits = (bits << np.uint32(1)) | (a < b).astype(np.uint32)
    out[ry:h - ry, rx:w - rx] = bits
    return out


def census(img, symmetric, cw, ch):
    return census_sym(img, cw, ch) if symmetric else census_centre(img, cw, ch)


def remap_q(img, xq, yq):
    """out = ((32-ax)(32-ay) p00 + ax (32-ay) p01 + (32-ax) ay p10 + ax ay p11 + 512) >> 10, taps outside the frame 0"""
    img = np.asarray(img)
    if img.ndim == 3:
        return np.stack([remap_q(f, xq, yq) for f in img])
    h, w = img.shape
    assert xq.shape == (h, w) and yq.shape == (h, w)
    xq, yq = xq.astype(np.int64), yq.astype(np.int64)
    x0, y0 = xq >> 5, yq >> 5
    ax, ay = xq & 31, yq & 31

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)

    acc = ((32 - ax) * (32 - ay) * tap(y0, x0) + ax * (32 - ay) * tap(y0, x0 + 1) + (32 - ax) * ay * tap(y0 + 1, x0) +
           ax * ay * tap(y0 + 1, x0 + 1) + 512)
    assert acc.min() >= 0 and acc.max() < 2 ** 32                 # the kernel's unsigned 32-bit accumulator
    out = acc >> 10
    assert out.max() <= np.iinfo(img.dtype).max
    return out.astype(img.dtype)


def remap(img, map_x, map_y):
    return remap_q(img, *RR.quantise(map_x, map_y))


def rank_pair(left, right):
    """(left, right) as uint8 dense ranks over the values of BOTH images: a < b, a == b, a > b hold between any two samples of the
    pair exactly where they hold between their ranks"""
    values = np.unique(np.concatenate([np.asarray(left).ravel(), np.asarray(right).ravel()]))
    assert values.size <= 256, values.size
    return (np.searchsorted(values, left).astype(np.uint8), np.searchsorted(values, right).astype(np.uint8))


def lut_pair(left8, right8, bits, seed):
    """v = lut[u8]: lut strictly increasing, random, below 2^bits with steps from 1 upwards, so that v >> (bits - 8) collapses
    neighbours the census of v still separates"""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    # 256 distinct values: a sorted sample without replacement of a range that is dense at the bottom (steps of 1 and 2 there)
    low = np.sort(rng.choice(np.arange(0, 512), 192, replace=False))
    high = np.sort(rng.choice(np.arange(512, top + 1), 64, replace=False))
    lut = np.concatenate([low, high]).astype(np.uint16)
    assert lut.size == 256 and np.all(np.diff(lut.astype(np.int64)) > 0) and int(lut[-1]) <= top
    return lut[np.asarray(left8, np.uint8)], lut[np.asarray(right8, np.uint8)]
