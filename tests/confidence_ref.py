"""The matching confidence of include/sgm_mi355x.h (SGM_MatchConfidence) restated in numpy, for one view of one frame.

confidence(S, dmin, right) takes the aggregated costs S, u16 [H][W][D] (index k = d - dmin), and returns (m1, m2, d1, conf):
  left view:  costs of pixel (y, x) = S[y][x][k];  right view: S[y][x + dmin + k][k], 65535 where that column is off the image.
  m1 = smallest cost; d1 = first index reaching it (-1 if nothing beats 65535, the reference's strict '>' from 65535);
  m2 = smallest cost over every index != d1 (65535 if there is none);
  conf = 0 if m2 == 0 else floor((m2 - m1) * 65535 / m2)   (unsigned 32-bit).
wta(...) is the reference's winner-take-all finish on those numbers (SemiGlobalMatching.c:412-440), used to tie them to the
oracle's disparity maps."""
import numpy as np

INF = np.float32(np.inf)


def view_costs(S, dmin=0, right=False):
    """The [H][W][D] costs of every reference-view pixel (u32, 65535 off the image)."""
    S = np.asarray(S, np.uint32)
    if not right:
        return S
    h, w, d = S.shape
    out = np.full((h, w, d), 65535, np.uint32)
    for k in range(d):
        lo = dmin + k                                   # column x + dmin + k of the left view
        n = w - lo
        if n > 0:
            out[:, :n, k] = S[:, lo:, k]
    return out


def confidence(S, dmin=0, right=False):
    c = view_costs(S, dmin, right)
    h, w, d = c.shape
    m1 = c.min(axis=2)
    d1 = np.argmax(c == m1[..., None], axis=2).astype(np.int64)      # first index reaching m1
    d1[m1 >= 65535] = -1                                             # nothing beat 65535
    others = c.copy()
    yy, xx = np.nonzero(d1 >= 0)
    others[yy, xx, d1[yy, xx]] = 65535 + 1                           # excluded (above every real cost)
    m2 = others.min(axis=2) if d > 0 else np.full((h, w), 65535, np.uint32)
    m2 = np.minimum(m2, 65535).astype(np.uint32)
    m1 = m1.astype(np.uint32)
    conf = np.zeros((h, w), np.uint32)
    nz = m2 != 0
    conf[nz] = ((m2[nz] - m1[nz]) * np.uint32(65535)) // m2[nz]
    return m1, m2, d1, conf.astype(np.uint16)


def wta(S, m1, m2, d1, dmin, dmax, unique, ratio, right=False):
    """The disparity map the reference's ComputeDisparity makes from m1 / m2 / d1 (uniqueness .c:412-426, border .c:428,
    sub-pixel .c:430-440; float32 arithmetic as the C)."""
    c = view_costs(S, dmin, right)
    h, w, D = c.shape
    k = np.asarray(d1, np.int64)
    best = np.asarray(m1, np.int64)
    ok = k >= 0                                                      # no candidate: +INF whatever the options
    if unique:
        keep = np.float32(1) - np.float32(ratio)
        margin = (best.astype(np.float32) * keep).astype(np.uint16).astype(np.int64)
        ok &= (np.asarray(m2, np.int64) - best) > margin
    ok &= (k != 0) & (k != D - 1)
    kk = np.clip(k, 1, max(D - 2, 1))[..., None]
    c1 = np.take_along_axis(c, kk - 1, axis=2)[..., 0].astype(np.uint16).view(np.int16).astype(np.int64)   # 65535 -> -1
    c2 = np.take_along_axis(c, np.minimum(kk + 1, D - 1), axis=2)[..., 0].astype(np.uint16).view(np.int16).astype(np.int64)
    denom = (c1 + c2 - 2 * best).astype(np.int16).astype(np.int64)
    denom[denom < 1] = 1
    val = (k + dmin).astype(np.float32) + (c1 - c2).astype(np.float32) / (denom.astype(np.float32) * np.float32(2.0))
    return np.where(ok, val, INF).astype(np.float32)
