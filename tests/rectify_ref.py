"""Restatement of the rectification contract of include/sgm_mi355x.h (SGM_SetRectify), numpy, integers only for the sampling.

    quantise(map_x, map_y)          -> (xq, yq) int32: q = floor(m * 32 + 0.5); a pixel with a coordinate that is not finite or has
                                       |m| > 32768 gets (-64, -64), all four taps outside
    remap(img, map_x, map_y)        -> the image (or [B][H][W] batch) sampled through float32 maps [H][W]
    remap_q(img, xq, yq)            -> the same from quantised maps
    maps(K, dist, R, Knew, w, h)    -> (map_x, map_y) float32 by the formulas of OpenCV's initUndistortRectifyMap, in double
"""
import numpy as np


def quantise(map_x, map_y):
    mx = np.asarray(map_x, np.float32).astype(np.float64)
    my = np.asarray(map_y, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(mx) & np.isfinite(my) & ~(np.abs(mx) > 32768.0) & ~(np.abs(my) > 32768.0)
    xq = np.full(mx.shape, -64, np.int32)
    yq = np.full(mx.shape, -64, np.int32)
    xq[ok] = np.floor(mx[ok] * 32.0 + 0.5).astype(np.int32)
    yq[ok] = np.floor(my[ok] * 32.0 + 0.5).astype(np.int32)
    return xq, yq


def remap_q(img, xq, yq):
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 3:
        return np.stack([remap_q(f, xq, yq) for f in img])
    h, w = img.shape
    assert xq.shape == (h, w) and yq.shape == (h, w)
    xq = xq.astype(np.int64)
    yq = yq.astype(np.int64)
    x0, y0 = xq >> 5, yq >> 5                                   # arithmetic shifts: floor
    ax, ay = xq & 31, yq & 31

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
        return np.where(inside, v, 0)

    acc = ((32 - ax) * (32 - ay) * tap(y0, x0) + ax * (32 - ay) * tap(y0, x0 + 1) + (32 - ax) * ay * tap(y0 + 1, x0) +
           ax * ay * tap(y0 + 1, x0 + 1) + 512) >> 10
    assert acc.min() >= 0 and acc.max() <= 255
    return acc.astype(np.uint8)


def remap(img, map_x, map_y):
    return remap_q(img, *quantise(map_x, map_y))


def maps(K, dist, R, Knew, width, height):
    K, R, Knew = (np.asarray(m, np.float64).reshape(3, 3) for m in (K, R, Knew))
    k1, k2, p1, p2, k3 = (float(v) for v in np.asarray(dist, np.float64).reshape(5))
    iR = np.linalg.inv(Knew @ R)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    X = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    Y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    Wz = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    x, y = X / Wz, Y / Wz
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return (K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32)


def rotation_z(degrees):
    """rotation about the optical axis by `degrees`"""
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def camera(width, height, focal=None):
    """a plain camera matrix: principal point in the frame's centre"""
    f = float(focal if focal else max(width, height))
    return np.array([[f, 0.0, (width - 1) / 2.0], [0.0, f, (height - 1) / 2.0], [0.0, 0.0, 1.0]])


# the models the tests share: (dist, rotation about z in degrees, focal length of Knew / that of K)
PLAIN = ((0.0, 0.0, 0.0, 0.0, 0.0), 0.0, 1.0)
RADIAL = ((-0.3, 0.1, 0.01, -0.005, 0.0), 0.0, 0.7)     # strongly radial, with tangential terms; zoomed out: taps beyond all four borders
ROTATED = ((0.02, 0.0, 0.0, 0.0, 0.0), 7.0, 1.0)
SMALL = ((-0.08, 0.02, 0.001, -0.001, 0.0), 1.5, 1.0)   # a small rotation plus radial: what a real rig's maps look like


def model(m, width, height, sign=1.0):
    """(K, dist, R, Knew) of one of the models above; sign: the sense of its rotation"""
    dist, deg, zoom = m
    K = camera(width, height)
    Knew = K.copy()
    Knew[0, 0] *= zoom
    Knew[1, 1] *= zoom
    return K, np.array(dist), rotation_z(sign * deg), Knew


def model_maps(m, width, height, sign=1.0):
    return maps(*model(m, width, height, sign), width, height)
