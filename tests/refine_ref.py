"""The refinement of include/sgm_mi355x.h (SGM_SetRefine) restated in numpy: the Fast Global Smoother (Min et al. 2014) of a
disparity map D (f32 [B][H][W] or [H][W], +INF invalid), weighted by the matching confidence K (u16) and guided by the grey image
G (u8), solved with the Thomas algorithm line by line in exactly the header's order.  Every operation is a separate float32
numpy operation (no contraction, correctly rounded divide, subnormals kept), so the result is bit-comparable with the kernels.

tables(lam, sigma, T, lib=None): the weight tables L_t of every iteration.  The library's sgm_refine_table when a library is
given (glibc's exp and numpy's may differ in the last bit), else numpy's own (table_numpy)."""
import ctypes as C

import numpy as np

F = np.float32
INF = F(np.inf)


def table_numpy(lam, sigma, T, t):
    """L_t[k] = (float)(lam_t * exp(-k / sigma)), lam_t = lambda * 1.5 * 4^(T-1-t) / (4^T - 1), in double, rounded once."""
    lam_t = float(F(lam)) * 1.5 * 4.0 ** (T - 1 - t) / (4.0 ** T - 1.0)
    k = np.arange(256, dtype=np.float64)
    return (lam_t * np.exp(-k / float(F(sigma)))).astype(F)


def table_lib(lib, lam, sigma, T, t):
    f = lib.sgm_refine_table
    f.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
    f.restype = C.c_bool
    out = np.zeros(256, F)
    if not f(lam, sigma, T, t, out.ctypes.data):
        raise ValueError(f"sgm_refine_table refused ({lam}, {sigma}, {T}, {t})")
    return out


def tables(lam, sigma, T, lib=None):
    return [table_lib(lib, lam, sigma, T, t) if lib is not None else table_numpy(lam, sigma, T, t) for t in range(T)]


def solve_lines(g, U, V, L):
    """One tridiagonal solve per line (axis 1) for both right-hand sides: g u8 [N][n], U / V f32 [N][n], L f32 [256].
    Returns (x_U, x_V)."""
    N, n = g.shape
    gi = g.astype(np.int32)
    e = L[np.abs(gi[:, 1:] - gi[:, :-1])] if n > 1 else np.zeros((N, 0), F)
    z = np.zeros((N, 1), F)
    a = np.concatenate([z, e], axis=1)                       # a_i = e_{i-1}, 0 at i = 0
    c = np.concatenate([e, z], axis=1)                       # c_i = e_i, 0 at i = n-1
    b = (F(1) + a) + c
    q = np.empty((N, n), F)
    ru = np.empty((N, n), F)
    rv = np.empty((N, n), F)
    m = b[:, 0]
    q[:, 0] = c[:, 0] / m
    ru[:, 0] = U[:, 0] / m
    rv[:, 0] = V[:, 0] / m
    for i in range(1, n):
        ai = a[:, i]
        m = b[:, i] - ai * q[:, i - 1]
        q[:, i] = c[:, i] / m
        ru[:, i] = (U[:, i] + ai * ru[:, i - 1]) / m
        rv[:, i] = (V[:, i] + ai * rv[:, i - 1]) / m
    xu = np.empty((N, n), F)
    xv = np.empty((N, n), F)
    xu[:, n - 1] = ru[:, n - 1]
    xv[:, n - 1] = rv[:, n - 1]
    for i in range(n - 2, -1, -1):
        xu[:, i] = ru[:, i] + q[:, i] * xu[:, i + 1]
        xv[:, i] = rv[:, i] + q[:, i] * xv[:, i + 1]
    return xu, xv


def refine(D, K, G, tabs, keep_invalid=False):
    """The refined map of D (same shape) with the weight tables `tabs` (one per iteration, see tables())."""
    D = np.asarray(D, F)
    shape = D.shape
    D3 = D.reshape((-1,) + shape[-2:])
    K3 = np.asarray(K, np.uint16).reshape(D3.shape)
    G3 = np.asarray(G, np.uint8).reshape(D3.shape)
    B, H, W = D3.shape
    ok = np.isfinite(D3)
    c = np.where(ok, K3.astype(F) / F(65535), F(0)).astype(F)
    U = np.where(ok, c * np.where(ok, D3, F(0)), F(0)).astype(F)
    V = c
    grow = G3.reshape(B * H, W)
    gcol = np.ascontiguousarray(G3.transpose(0, 2, 1)).reshape(B * W, H)
    for L in tabs:
        L = np.asarray(L, F)
        u, v = solve_lines(grow, U.reshape(B * H, W), V.reshape(B * H, W), L)
        U, V = u.reshape(B, H, W), v.reshape(B, H, W)
        ut = np.ascontiguousarray(U.transpose(0, 2, 1)).reshape(B * W, H)
        vt = np.ascontiguousarray(V.transpose(0, 2, 1)).reshape(B * W, H)
        u, v = solve_lines(gcol, ut, vt, L)
        U = np.ascontiguousarray(u.reshape(B, W, H).transpose(0, 2, 1))
        V = np.ascontiguousarray(v.reshape(B, W, H).transpose(0, 2, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(V > 0, U / np.where(V > 0, V, F(1)), INF).astype(F)
    if keep_invalid:
        out[~ok] = INF
    return out.reshape(shape)
