"""Rectification (extension; the contract is in include/sgm_mi355x.h, SGM_SetRectify) without a GPU: the numpy restatement's own
properties, the map builder sgm_rectify_maps against it, the C host's logic on the stand-in device (tests/stub_device.c +
tests/stub_rectify.c), a sanitizer run of a stand-alone driver, and what rectification is for: the cone pair, taken through two
camera rotations, matches again once it is rectified."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rectify_ref as RR
import standin
from conftest import ROOT, case_inputs, load_npz, option_from_dict

STUB_RECTIFY = os.path.join(ROOT, "tests", "stub_rectify.c")
_p, _i, _b = C.c_void_p, C.c_int, C.c_bool


def identity(w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x, y


def noise(w, h, seed=1, frames=None):
    shape = (h, w) if frames is None else (frames, h, w)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(70, 33), (20, 31), (1, 1)])
def test_identity_maps_return_the_image(w, h):
    img = noise(w, h)
    assert np.array_equal(RR.remap(img, *identity(w, h)), img)


def test_integer_shift_copies_pixels_with_a_zero_border():
    w, h = 40, 24
    img = noise(w, h) | 1                                        # no zero inside: the border is told apart
    x, y = identity(w, h)
    got = RR.remap(img, x + 3, y - 2)
    want = np.zeros_like(img)
    want[2:, :w - 3] = img[:h - 2, 3:]
    assert np.array_equal(got, want)


def test_half_pixel_in_x_is_the_rounded_mean():
    w, h = 33, 9
    img = noise(w, h)
    x, y = identity(w, h)
    xq, yq = RR.quantise(x + 0.5, y)
    assert np.all((xq & 31) == 16) and np.all((yq & 31) == 0)
    got = RR.remap(img, x + 0.5, y)
    p00 = img.astype(np.int64)
    p01 = np.concatenate([p00[:, 1:], np.zeros((h, 1), np.int64)], axis=1)
    assert np.array_equal(got, ((p00 + p01 + 1) >> 1).astype(np.uint8))


def test_all_255_stays_255_in_the_interior():
    """The accumulator's worst case: every weight pair (ax, ay) on four taps of 255 sums to 1024 * 255 and rounds to 255."""
    w, h = 70, 40
    img = np.full((h, w), 255, np.uint8)
    x, y = identity(w, h)
    fx, fy = x + (x % 32) / 32, y + (y % 32) / 32                # all 1024 weight pairs
    xq, yq = RR.quantise(fx, fy)
    assert len({(a, b) for a, b in zip((xq & 31).ravel().tolist(), (yq & 31).ravel().tolist())}) == 1024
    got = RR.remap(img, fx, fy)
    inside = ((xq >> 5) + 1 < w) & ((yq >> 5) + 1 < h)
    assert inside.sum() > 0.9 * w * h and np.all(got[inside] == 255)
    rng = np.random.default_rng(3)
    rx, ry = (rng.uniform(0, w - 1.01, (h, w)).astype(np.float32), rng.uniform(0, h - 1.01, (h, w)).astype(np.float32))
    assert np.all(RR.remap(img, rx, ry) == 255)


def test_non_finite_and_huge_map_values_give_zero():
    w, h = 16, 8
    img = np.full((h, w), 200, np.uint8)
    x, y = identity(w, h)
    bad = [np.nan, np.inf, -np.inf, 1e9, -1e9, 32768.5, -40000.0]
    for k, v in enumerate(bad):
        x[k % h, k] = v                                          # a bad x with a good y ...
        y[(k + 3) % h, k + 8] = v                                # ... and a good x with a bad y: both coordinates go
    xq, yq = RR.quantise(x, y)
    got = RR.remap(img, x, y)
    for k in range(len(bad)):
        for r, c in ((k % h, k), ((k + 3) % h, k + 8)):
            assert (xq[r, c], yq[r, c]) == (-64, -64) and got[r, c] == 0
    assert (got == 0).sum() == 2 * len(bad)
    # |m| == 32768 is still quantised (and far outside)
    x2, y2 = identity(w, h)
    x2[0, 0] = 32768.0
    assert RR.quantise(x2, y2)[0][0, 0] == 32768 * 32 and RR.remap(img, x2, y2)[0, 0] == 0


def test_taps_are_decided_one_by_one_at_the_border():
    img = np.array([[100, 200], [50, 250]], np.uint8)
    x, y = identity(2, 2)
    # half a pixel left of column 0: the outside tap counts as 0 -> (0 + 100 + 1) >> 1
    assert RR.remap(img, x - 0.5, y)[0, 0] == 50
    # half a pixel below the last row, at column 1: (250 + 0 + 1) >> 1
    assert RR.remap(img, x, y + 0.5)[1, 1] == 125
    assert RR.remap(img, x - 1.0, y)[0, 0] == 0 and RR.remap(img, x - 1.0, y)[0, 1] == 100


# ---- the map builder ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


def lib_maps(lib, K, dist, R, Knew, w, h):
    f = lib.sgm_rectify_maps
    f.argtypes, f.restype = [_p] * 4 + [_i, _i, _p, _p], _b
    arrs = [np.ascontiguousarray(m, np.float64) for m in (K, dist, R, Knew)]
    mx, my = np.full((h, w), -7, np.float32), np.full((h, w), -7, np.float32)
    ok = f(*(a.ctypes.data for a in arrs), w, h, mx.ctypes.data, my.ctypes.data)
    return (mx, my) if ok else None


def ulps(a, b):
    """distance in float32 steps (finite values of one sign or near zero)"""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(np.ascontiguousarray(a, np.float32)) - key(np.ascontiguousarray(b, np.float32)))


@pytest.mark.parametrize("name", ["PLAIN", "RADIAL", "ROTATED"])
@pytest.mark.parametrize("w,h", [(70, 33), (450, 375)])
def test_map_builder_agrees_with_the_restatement(lib, name, w, h):
    """Both sides are double arithmetic rounded once to float32; a different operation order moves the double by ~1e-12 px, so a
    value lands on the same float32 or, at a rounding boundary, on its neighbour: one ulp."""
    args = RR.model(getattr(RR, name), w, h)
    got = lib_maps(lib, *args, w, h)
    want = RR.maps(*args, w, h)
    assert got is not None
    for g, t in zip(got, want):
        assert np.all(np.isfinite(g))
        worst = int(ulps(g, t).max())
        print(f"{name} {w}x{h}: worst distance {worst} ulp, {int((ulps(g, t) > 0).sum())} of {g.size} values differ")
        assert worst <= 1


def test_map_builder_identity_is_exact(lib):
    w, h = 70, 33
    K = RR.camera(w, h)
    got = lib_maps(lib, K, np.zeros(5), np.eye(3), K, w, h)
    x, y = identity(w, h)
    xq, yq = RR.quantise(*got)
    assert np.array_equal(xq, (x * 32).astype(np.int32)) and np.array_equal(yq, (y * 32).astype(np.int32))
    img = noise(w, h)
    assert np.array_equal(RR.remap(img, *got), img)


def test_map_builder_refusals(lib):
    w, h = 8, 4
    K = RR.camera(w, h)
    d0, I3 = np.zeros(5), np.eye(3)
    assert lib_maps(lib, K, d0, I3, K, w, h) is not None
    assert lib_maps(lib, K, d0, I3, np.zeros((3, 3)), w, h) is None                   # singular Knew R
    assert lib_maps(lib, K, d0, np.array([[1, 0, 0], [2, 0, 0], [0, 0, 1.0]]), K, w, h) is None
    f = lib.sgm_rectify_maps
    arrs = [np.ascontiguousarray(m, np.float64) for m in (K, d0, I3, K)]
    out = np.zeros((h, w), np.float32)
    ptr = [a.ctypes.data for a in arrs]
    for bad_w, bad_h in ((0, h), (w, 0), (-1, h)):
        assert not f(*ptr, bad_w, bad_h, out.ctypes.data, out.ctypes.data)
    for k in range(4):
        assert not f(*(None if j == k else p for j, p in enumerate(ptr)), w, h, out.ctypes.data, out.ctypes.data)
    assert not f(*ptr, w, h, None, out.ctypes.data) and not f(*ptr, w, h, out.ctypes.data, None)


def test_python_wrapper_and_header(lib):
    import soc_project_stereo_matching_amd as S
    w, h = 20, 31
    args = RR.model(RR.ROTATED, w, h)
    got = S.rectify_maps(*args, w, h)
    want = lib_maps(lib, *args, w, h)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for sym in ("SGM_SetRectify", "sgm_set_rectify", "sgm_rectify", "sgm_rectify_maps", "sgmd_remap"):
        assert hasattr(lib, sym), sym
    for m in ("set_rectify", "rectify", "read_rectified"):
        assert callable(getattr(S.SGMInstance, m, None)), m
    assert callable(getattr(S.SGM, "set_rectify", None)) and (S.STAGE_RECT_LEFT, S.STAGE_RECT_RIGHT) == (19, 20)
    assert "rect" not in " ".join(S.STAGE_NAMES)                  # read_stages() is what it was
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    for decl in (r"bool\s+SGM_SetRectify\(int width, int height, const float\* map_lx, const float\* map_ly, const float\* map_rx, const float\* map_ry\)",
                 r"bool\s+sgm_rectify\(sgm_instance\* s, const uint8_t\* d_left, const uint8_t\* d_right, uint8_t\* d_out_left, uint8_t\* d_out_right\)",
                 r"bool\s+sgm_rectify_maps\(const double K\[9\], const double dist\[5\], const double R\[9\], const double Knew\[9\], int width, int height,"):
        assert re.search(decl, text), decl
    assert "floor((double)m * 32.0 + 0.5)" in text and "+ 512) >> 10" in text


# ---- host logic on the stand-in device ---------------------------------------------------------------------------------

def _sign(L):
    for name, (res, args) in {"sgm_set_rectify": (_b, [_p, _i, _i] + [_p] * 4), "SGM_SetRectify": (_b, [_i, _i] + [_p] * 4),
                              "sgm_rectify": (_b, [_p] * 5), "sgm_match_planes": (_b, [_p, _p, C.c_float, C.c_float, C.c_float, _p]),
                              "SGM_Initialize": (_b, [C.c_uint16, C.c_uint16, _p]), "SGM_Reset": (_b, [C.c_uint16, C.c_uint16, _p]),
                              "SGM_Match": (_b, [_p] * 3), "SGM_Shutdown": (None, []),
                              "stub_remap_ptr": (_p, [_i, _i]), "stub_remap_count": (_i, []), "stub_remap_frames": (_i, [_i]),
                              "stub_remap_fail_at": (None, [_i]), "stub_fail_alloc_at": (None, [_i]), "stub_alloc_count": (_i, [])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("rectstub"), extra_sources=[STUB_RECTIFY], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("rectstub_without")))


W, H = 48, 20


class Frame:
    def __init__(self, w=W, h=H, seed=5):
        self.left, self.right = noise(w, h, seed), noise(w, h, seed + 1)
        self.out, self.out_r = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        self.conf = np.zeros((h, w), np.uint16)
        self.planes = noise(w, h, seed + 2, frames=6)

    def args(self):
        return self.left.ctypes.data, self.right.ctypes.data, self.out.ctypes.data


class Maps:
    def __init__(self, w=W, h=H, shift=0.0):
        self.lx, self.ly = RR.model_maps(RR.SMALL, w, h)
        self.rx, self.ry = RR.model_maps(RR.SMALL, w, h, sign=-1.0)
        self.lx = self.lx + np.float32(shift)
        self.w, self.h = w, h

    def args(self):
        return (self.w, self.h) + tuple(np.ascontiguousarray(m, np.float32).ctypes.data for m in (self.lx, self.ly, self.rx, self.ry))

    def quantised(self):
        """the device lay-out: [view][xq, yq][pitch]"""
        n = self.w * self.h
        pitch = (n + 3) & ~3
        q = np.full((2, 2, pitch), -64, np.int32)
        for v, (mx, my) in enumerate(((self.lx, self.ly), (self.rx, self.ry))):
            xq, yq = RR.quantise(mx, my)
            q[v, 0, :n], q[v, 1, :n] = xq.ravel(), yq.ravel()
        return q


def make(L, maps=None):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    if maps is not None:
        m = (maps.lx, maps.ly, maps.rx, maps.ry)                 # keep the arrays alive over the call
        assert L.sgm_set_rectify(s, *maps.args()), m[0].shape
    return s, S.default_option(16)


def device_bytes(ptr, n):
    return np.frombuffer((C.c_uint8 * n).from_address(ptr), np.uint8).copy()


def test_one_remap_per_match_of_every_kind(host):
    L = host
    maps = Maps()
    s, opt = make(L, maps)
    f = Frame()
    kinds = {
        "plain": lambda: L.sgm_match(s, *f.args()),
        "confidence": lambda: L.sgm_match_confidence(s, *f.args(), f.conf.ctypes.data),
        "both": lambda: L.sgm_match_both(s, *f.args(), f.out_r.ctypes.data),
        "planes": lambda: L.sgm_match_planes(s, f.planes.ctypes.data, 700.0, 160.0, 0.0, f.out.ctypes.data),
        "device": lambda: L.sgm_match_device(s, *f.args()) and L.sgm_synchronize(s),
        "confidence_device": lambda: L.sgm_match_confidence_device(s, *f.args(), f.conf.ctypes.data) and L.sgm_synchronize(s),
        "both_device": lambda: L.sgm_match_both_device(s, *f.args(), f.out_r.ctypes.data) and L.sgm_synchronize(s),
    }
    for name, run in kinds.items():
        assert L.sgm_reset(s, W, H, C.byref(opt)), name
        L.stub_clear()
        L.stub_remap_clear()
        assert run(), name
        assert L.stub_remap_count() == 1, name
        src_l, src_r, out_l, out_r = (L.stub_remap_ptr(0, k) for k in (1, 2, 3, 4))
        # the remap writes the instance's own buffers, never the caller's images
        assert out_l not in (src_l, src_r, f.left.ctypes.data, f.right.ctypes.data) and out_l != out_r, name
        assert out_r not in (src_l, src_r, f.left.ctypes.data, f.right.ctypes.data), name
        if "device" in name:
            assert (src_l, src_r) == (f.left.ctypes.data, f.right.ctypes.data), name    # read in place
        # ... and what it wrote is the restatement's remap of what it read (the stand-in samples for real)
        if name != "planes":
            assert np.array_equal(device_bytes(out_l, W * H).reshape(H, W), RR.remap(f.left, maps.lx, maps.ly)), name
            assert np.array_equal(device_bytes(out_r, W * H).reshape(H, W), RR.remap(f.right, maps.rx, maps.ry)), name
        # the remap comes first: the stand-in's own log starts with the census
        order = [n for n, _ in standin.launches(L) if n not in ("gray",)]
        assert order[0] in ("census", "d2d"), (name, order[:3])
    L.sgm_destroy(s)


def test_uploaded_maps_are_the_quantised_maps(host):
    L = host
    maps = Maps()
    s, opt = make(L, maps)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    f = Frame()
    L.stub_remap_clear()
    assert L.sgm_match(s, *f.args())
    want = maps.quantised()
    got = np.frombuffer((C.c_int32 * want.size).from_address(L.stub_remap_ptr(0, 0)), np.int32).reshape(want.shape)
    assert np.array_equal(got, want)
    L.sgm_destroy(s)


def test_off_means_no_remap_and_the_launch_log_of_a_host_without_it(host, host_without):
    f = Frame()
    logs = []
    for L in (host, host_without):
        s, opt = make(L)
        L.stub_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *f.args())
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, *f.args(), f.conf.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])    # allocations and their sizes included
        L.sgm_destroy(s)
    assert logs[0] == logs[1]
    # on against off: the remap has a log of its own, the launches are the same
    L = host
    maps = Maps()
    s, opt = make(L, maps)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    L.stub_clear(); L.stub_remap_clear()
    assert L.sgm_match(s, *f.args())
    on = standin.launches(L)
    assert L.stub_remap_count() == 1
    assert L.sgm_set_rectify(s, 0, 0, None, None, None, None)     # off with NULL: the other arguments are not looked at
    assert L.sgm_reset(s, W, H, C.byref(opt))
    L.stub_clear(); L.stub_remap_clear()
    assert L.sgm_match(s, *f.args())
    assert L.stub_remap_count() == 0
    assert standin.launches(L) == on
    assert L.sgm_read_stage(s, 19, f.left.ctypes.data, W * H) == 0 and L.sgm_read_stage(s, 20, f.left.ctypes.data, W * H) == 0
    assert not L.sgm_rectify(s, f.left.ctypes.data, f.right.ctypes.data, f.conf.ctypes.data, f.out.ctypes.data)
    L.sgm_destroy(s)


def test_setter_validation_changes_nothing(host):
    L = host
    maps = Maps()
    s, opt = make(L, maps)
    w, h, lx, ly, rx, ry = maps.args()
    for bad in ((w, h, lx, None, rx, ry), (w, h, lx, ly, None, ry), (w, h, lx, ly, rx, None), (0, h, lx, ly, rx, ry),
                (w, 0, lx, ly, rx, ry), (-3, h, lx, ly, rx, ry)):
        assert not L.sgm_set_rectify(s, *bad), bad
        assert not L.SGM_SetRectify(*bad), bad
    assert not L.sgm_set_rectify(None, w, h, lx, ly, rx, ry)
    assert L.sgm_reset(s, W, H, C.byref(opt))                     # the maps set before are still in effect
    f = Frame()
    L.stub_remap_clear()
    assert L.sgm_match(s, *f.args()) and L.stub_remap_count() == 1
    L.sgm_destroy(s)


def test_initialize_refuses_a_shape_mismatch_and_row_tiles(host):
    L = host
    s, opt = make(L, Maps())
    assert not L.sgm_reset(s, W + 1, H, C.byref(opt)) and not L.sgm_initialize(s, W, H - 1, C.byref(opt))
    assert not L.sgm_match(s, *Frame().args())                    # not initialized
    assert L.sgm_reset(s, W, H, C.byref(opt))
    assert L.sgm_set_rows(s, 4, 12)
    assert not L.sgm_reset(s, W, H, C.byref(opt))
    assert L.sgm_set_rectify(s, 0, 0, None, None, None, None)
    assert L.sgm_reset(s, W, H, C.byref(opt))                     # row tiles without rectification: as ever
    assert L.sgm_set_rows(s, 0, 0)
    L.sgm_destroy(s)


def test_new_maps_take_effect_at_the_next_reset(host):
    L = host
    a, b = Maps(), Maps(shift=2.0)
    s, opt = make(L, a)
    f = Frame()
    assert L.sgm_reset(s, W, H, C.byref(opt))
    L.stub_clear()
    assert L.sgm_reset(s, W, H, C.byref(opt))                     # unchanged maps: nothing is uploaded again
    assert "h2d" not in [e.name for e in standin.log(L)]
    assert L.sgm_set_rectify(s, *b.args())
    L.stub_remap_clear()
    assert L.sgm_match(s, *f.args())                              # not before a reset
    assert np.array_equal(device_bytes(L.stub_remap_ptr(0, 3), W * H).reshape(H, W), RR.remap(f.left, a.lx, a.ly))
    L.stub_clear()
    assert L.sgm_reset(s, W, H, C.byref(opt))
    assert [e.arg for e in standin.log(L) if e.name == "h2d"] == [b.quantised().nbytes]
    L.stub_remap_clear()
    assert L.sgm_match(s, *f.args())
    assert np.array_equal(device_bytes(L.stub_remap_ptr(0, 3), W * H).reshape(H, W), RR.remap(f.left, b.lx, b.ly))
    # the caller's arrays were not borrowed: a bigger shape re-allocates everything and uploads from the host's copy
    w2, h2 = W + 8, H + 4
    c = Maps(w2, h2)
    assert L.sgm_set_rectify(s, *c.args())
    want = c.quantised()
    for m in (c.lx, c.ly, c.rx, c.ry):
        m[:] = np.nan
    assert L.sgm_reset(s, w2, h2, C.byref(opt))
    f2 = Frame(w2, h2)
    L.stub_remap_clear()
    assert L.sgm_match(s, *f2.args())
    got = np.frombuffer((C.c_int32 * want.size).from_address(L.stub_remap_ptr(0, 0)), np.int32).reshape(want.shape)
    assert np.array_equal(got, want)
    L.sgm_destroy(s)


def test_batches_and_the_stand_alone_form(host):
    L = host
    maps = Maps()
    s, opt = make(L, maps)
    assert L.sgm_set_batch(s, 3) and L.sgm_reset(s, W, H, C.byref(opt))
    left, right = noise(W, H, 7, frames=3), noise(W, H, 8, frames=3)
    out = np.zeros((3, H, W), np.float32)
    L.stub_remap_clear()
    assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
    assert L.stub_remap_count() == 1 and L.stub_remap_frames(0) == 3
    assert np.array_equal(device_bytes(L.stub_remap_ptr(0, 4), 3 * W * H).reshape(3, H, W), RR.remap(right, maps.rx, maps.ry))
    ol, orr = np.zeros_like(left), np.zeros_like(right)
    assert L.sgm_rectify(s, left.ctypes.data, right.ctypes.data, ol.ctypes.data, orr.ctypes.data)
    assert np.array_equal(ol, RR.remap(left, maps.lx, maps.ly)) and np.array_equal(orr, RR.remap(right, maps.rx, maps.ry))
    for k in range(4):
        args = [left.ctypes.data, right.ctypes.data, ol.ctypes.data, orr.ctypes.data]
        args[k] = None
        assert not L.sgm_rectify(s, *args)
    # stages 19 / 20: the selected frame
    got = np.zeros((H, W), np.uint8)
    L.sgm_select_frame.argtypes = [_p, _i]
    L.sgm_select_frame(s, 2)
    assert L.sgm_read_stage(s, 19, got.ctypes.data, got.nbytes) == got.nbytes
    assert np.array_equal(got, RR.remap(left[2], maps.lx, maps.ly))
    assert L.sgm_read_stage(s, 20, got.ctypes.data, got.nbytes) == got.nbytes
    assert np.array_equal(got, RR.remap(right[2], maps.rx, maps.ry))
    assert L.sgm_read_stage(s, 19, got.ctypes.data, got.nbytes - 1) == 0
    L.sgm_destroy(s)


def test_refinement_guide_is_the_rectified_image(host):
    L = host
    s, opt = make(L, Maps())
    assert L.sgm_set_refine(s, 1, 16.0, 1.5, 1, 0) and L.sgm_reset(s, W, H, C.byref(opt))
    f = Frame()
    for right_view in (0, 1):
        L.sgm_set_reference_view(s, right_view)
        L.stub_clear(); L.stub_remap_clear()
        assert L.sgm_match(s, *f.args())
        rect = L.stub_remap_ptr(0, 4 if right_view else 3)
        copies = [e for e in standin.log(L) if e.name == "d2d" and e.arg == W * H]
        assert copies, "the guide copy"
        guide = standin.calls(L, "refine_pass")[0].b
        assert np.array_equal(device_bytes(guide, W * H), device_bytes(rect, W * H))
    L.sgm_destroy(s)


def test_refused_allocation_and_refused_remap_fail_cleanly(host):
    L = host
    f = Frame()
    maps = Maps()
    # every allocation of the first reset + match with rectification on, refused in turn
    s, opt = make(L, maps)
    n0 = L.stub_alloc_count()
    assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *f.args())
    total = L.stub_alloc_count() - n0
    L.sgm_destroy(s)
    assert total > 10
    for k in range(total):
        s, opt = make(L, maps)
        L.stub_fail_alloc_at(k)
        ok = L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *f.args())
        L.stub_fail_alloc_at(-1)
        assert not ok, k
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *f.args()), k      # and the instance recovers
        L.sgm_destroy(s)
    s, opt = make(L, maps)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    L.stub_clear(); L.stub_remap_clear()
    L.stub_remap_fail_at(0)
    assert not L.sgm_match(s, *f.args())
    assert "census" not in [e.name for e in standin.log(L)]       # nothing was queued behind the refused remap
    L.stub_remap_clear()
    assert L.sgm_match(s, *f.args()) and L.stub_remap_count() == 1
    L.sgm_destroy(s)


def test_default_instance_remembers_its_maps(host):
    L = host
    import soc_project_stereo_matching_amd as S
    opt = S.default_option(16)
    maps = Maps()
    f = Frame()
    assert L.SGM_SetRectify(*maps.args())
    try:
        L.stub_remap_clear()
        assert L.SGM_Initialize(W, H, C.byref(opt)) and L.SGM_Match(*f.args()) and L.stub_remap_count() == 1
        L.SGM_Shutdown()
        assert L.SGM_Reset(W, H, C.byref(opt)) and L.SGM_Match(*f.args()) and L.stub_remap_count() == 2
        assert np.array_equal(device_bytes(L.stub_remap_ptr(1, 3), W * H).reshape(H, W), RR.remap(f.left, maps.lx, maps.ly))
        assert L.SGM_SetRectify(0, 0, None, None, None, None)
        assert L.SGM_Reset(W, H, C.byref(opt)) and L.SGM_Match(*f.args()) and L.stub_remap_count() == 2
    finally:
        L.SGM_SetRectify(0, 0, None, None, None, None)
        L.SGM_Shutdown()


def test_host_without_the_launcher_links_and_refuses(host_without):
    L = host_without
    s, opt = make(L)
    maps = Maps()
    assert not L.sgm_set_rectify(s, *maps.args()) and not L.SGM_SetRectify(*maps.args())
    assert L.sgm_set_rectify(s, 0, 0, None, None, None, None) and L.SGM_SetRectify(0, 0, None, None, None, None)
    f = Frame()
    assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *f.args())
    assert not L.sgm_rectify(s, f.left.ctypes.data, f.right.ctypes.data, f.conf.ctypes.data, f.out.ctypes.data)
    L.sgm_destroy(s)


# ---- sanitizers on a stand-alone program -------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_rectify_host_is_asan_ubsan_clean(tmp_path):
    """tests/rectify_sanitize_driver.c: a program of its own, linked with the host, both stubs and the map builder."""
    exe = standin.build(tmp_path, sanitize=True, exe="rectify_sanitize_driver", flags=("-ffp-contract=off",),
                        extra_sources=[os.path.join(ROOT, "tests", "rectify_sanitize_driver.c"), STUB_RECTIFY])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("rectify_sanitize_driver ok")


# ---- what it is for: the cone pair through two camera rotations ----------------------------------------------------------

def bad_rate(d, gt, known):
    """share of the pixels with known ground truth whose disparity is +INF or off by more than 1 px"""
    bad = ~np.isfinite(d) | (np.abs(d - gt) > 1)
    return float(bad[known].mean())


def test_rectified_raw_pair_matches_like_the_original(oracle, golden_cases):
    """The cone pair (tests/golden/cone_im2.png / cone_im6.png as the grey images of cone_inputs.npz) seen by cameras rolled by +2
    and -1.5 degrees about the principal point -- warped with the restatement's own sampler through the analytic inverse -- no
    longer matches; rectified with maps from rectify_ref.maps() it matches nearly as the original does.  Bad pixels (> 1 px off
    or +INF) against the ground truth, measured: raw 97.24 %, rectified 18.91 %, original 16.76 %."""
    c = golden_cases["cone"]
    left, right = case_inputs(c, oracle)
    opt = option_from_dict(c["option"])
    h, w = left.shape
    K, d0 = RR.camera(w, h), np.zeros(5)
    raw, rect = [], []
    for img, deg in ((left, 2.0), (right, -1.5)):
        raw.append(RR.remap(img, *RR.maps(K, d0, RR.rotation_z(deg), K, w, h)))
        rect.append(RR.remap(raw[-1], *RR.maps(K, d0, RR.rotation_z(-deg), K, w, h)))
    z = load_npz("gt_disparity.npz")
    gt = z["cone"].astype(np.float32) / z["cone_scale"]
    known = z["cone"] > 0
    a, b, cc = (bad_rate(oracle.run(l, r, opt)["final"], gt, known) for l, r in (raw, rect, (left, right)))
    print(f"cone, bad > 1 px: raw pair {100 * a:.2f} %, rectified {100 * b:.2f} %, original pair {100 * cc:.2f} %")
    assert b < a
    assert abs(b - cc) < abs(b - a)
