"""Point clouds (extension; the contract is in include/sgm_mi355x.h, sgm_cloud_spec) without a GPU: the numpy restatement
tests/cloud_ref.py against a plain-Python double loop and against the depth conversion, header / library / Python agreement, the C
host's logic on the stand-in device (tests/stub_device.c + tests/stub_cloud.c), sgm_rectify_valid_mask against the rectification's
restatement, and a sanitizer run of a stand-alone driver.  Tolerance 0 everywhere."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import rectify_ref as RR
import standin
from conftest import ROOT, load_npz

STUB_CLOUD = os.path.join(ROOT, "tests", "stub_cloud.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
INF, NAN = float("inf"), float("nan")


FLT_ROUNDS_TO_INF = 3.4028235677973366e38                       # the largest float32 plus half a step: beyond it IEEE rounds to INF


def f32(v):
    """one rounding to float32 (IEEE, ties to even), as a Python float"""
    if not math.isfinite(v):
        return v
    if abs(v) >= FLT_ROUNDS_TO_INF:
        return math.copysign(INF, v)
    return struct.unpack("f", struct.pack("f", v))[0]


def div32(a, b):
    """float32 a / b, correctly rounded: the double quotient of two float32 values rounds to float32 without double rounding
    (53 >= 2 * 24 + 2 bits, Figueroa's theorem)"""
    return f32(a / b)


def loop_cloud(disp, s, mask=None, conf=None):
    """The definition of include/sgm_mi355x.h as a double loop over Python floats: sums, products and quotients of two float32
    values are exact or correctly rounded in double, so rounding each to float32 once is the float32 operation."""
    fb = f32(float(np.float32(s.fx)) * float(np.float32(s.baseline)))
    fx, fy, cx, cy, doffs = (float(np.float32(v)) for v in (s.fx, s.fy, s.cx, s.cy, s.doffs))
    z_min, z_max = float(np.float32(s.z_min)), float(np.float32(s.z_max))
    pts, offsets = [], [0]
    org = np.full((s.frames, s.height, s.width, 3), CR.QNAN, np.uint32)
    for f in range(s.frames):
        for y in range(s.height):
            for x in range(s.width):
                d = float(disp[f, y, x])
                if not math.isfinite(d):
                    continue
                if mask is not None and mask[f, y, x] == 0:
                    continue
                if conf is not None and int(conf[f, y, x]) < s.min_conf:
                    continue
                den = f32(d + doffs)
                if not math.isfinite(den) or not den > 0:
                    continue
                Z = div32(fb, den)
                if not math.isfinite(Z) or not (z_min <= Z <= z_max):
                    continue
                X = div32(f32(f32(x - cx) * Z), fx)
                Y = div32(f32(f32(y - cy) * Z), fy)
                pts.append((X, Y, Z, (y << 16) | x))
                org[f, y, x] = np.array([X, Y, Z], np.float32).view(np.uint32)
        offsets.append(len(pts))
    return np.array(pts, CR.POINT) if pts else np.empty(0, CR.POINT), np.array(offsets, np.uint32), org.view(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement -----------------------------------------------------------------------------------------------------

def hand_case():
    """7x5, two frames: every clause of the predicate decided by hand.  fb = 1000 * 2 = 2000, doffs = -1, 4 <= Z <= 500."""
    s = CR.spec(7, 5, fx=1000.0, fy=900.0, cx=3.25, cy=1.5, baseline=2.0, doffs=-1.0, frames=2, z_min=4.0, z_max=500.0, min_conf=300)
    d = np.full((2, 5, 7), 11.0, np.float32)                      # den 10 -> Z 200: kept
    mask = np.ones((2, 5, 7), np.uint8)
    conf = np.full((2, 5, 7), 65535, np.uint16)
    want = np.ones((2, 5, 7), bool)
    d[0, 0, 0], want[0, 0, 0] = INF, False
    d[0, 0, 1], want[0, 0, 1] = NAN, False
    d[0, 0, 2], want[0, 0, 2] = -INF, False
    d[0, 1, 0], want[0, 1, 0] = 1.0, False                        # den == 0
    d[0, 1, 1], want[0, 1, 1] = 0.5, False                        # den < 0 from the negative doffs
    d[0, 1, 2], want[0, 1, 2] = 501.0, True                       # den 500 -> Z == z_min exactly: kept
    d[0, 1, 3], want[0, 1, 3] = 5.0, True                         # den 4 -> Z == z_max exactly: kept
    d[0, 1, 4], want[0, 1, 4] = 4.9990234375, False               # just above z_max
    d[0, 1, 5], want[0, 1, 5] = 502.0, False                      # just below z_min
    mask[0, 2, 0], want[0, 2, 0] = 0, False
    mask[0, 2, 1], want[0, 2, 1] = 200, True                      # any non-zero byte
    conf[0, 2, 2], want[0, 2, 2] = 299, False                     # min_conf - 1
    conf[0, 2, 3], want[0, 2, 3] = 300, True                      # min_conf
    d[1, 4, 6], want[1, 4, 6] = 3e38, False                       # Z underflows below z_min
    return s, d, mask, conf, want


def test_restatement_equals_the_double_loop_on_hand_worked_cases():
    s, d, mask, conf, want = hand_case()
    keep, Z = CR.kept(d, s, mask, conf)
    assert np.array_equal(keep, want)
    assert Z[0, 1, 2] == 4.0 and Z[0, 1, 3] == 500.0 and Z[0, 2, 1] == 200.0
    pts, off, org = loop_cloud(d, s, mask, conf)
    got_pts, got_off = CR.points(d, s, mask, conf)
    assert same_bits(got_pts, pts) and np.array_equal(got_off, off)
    assert same_bits(CR.organized(d, s, mask, conf), org)
    assert off.tolist() == [0, int(want[0].sum()), int(want.sum())]
    # without the side maps the two pixels they dropped come back
    assert CR.points(d, s)[1][-1] == want.sum() + 2
    assert same_bits(CR.points(d, s)[0], loop_cloud(d, s)[0])
    # raster order and the pixel word
    first = got_pts[0]
    assert first["pixel"] == (0 << 16) | 3 and first["z"] == 200.0
    assert np.all(np.diff(got_pts["pixel"][:off[1]].astype(np.int64)) > 0)
    # X of that pixel by hand: (3 - 3.25) * 200 / 1000
    assert first["x"] == np.float32(-0.05) and first["y"] == np.float32((0 - 1.5) * 200 / 900)


def test_quotient_that_overflows_is_dropped():
    """a tiny denominator under a huge fb: Z = +INF is not finite, whatever z_max says"""
    s = CR.spec(7, 5, fx=3e19, fy=1.0, cx=0.0, cy=0.0, baseline=1e19, doffs=0.0)     # fb = 3e38
    d = np.full((1, 5, 7), 2.0, np.float32)
    d[0, 0, 0] = 1e-3                                             # 3e41: overflow
    d[0, 0, 1] = 1e-40                                            # a subnormal denominator
    d[0, 0, 2] = 0.9                                              # 3.33e38: still finite
    keep, Z = CR.kept(d, s)
    assert not keep[0, 0, 0] and not keep[0, 0, 1] and keep[0, 0, 2] and np.isinf(Z[0, 0, 0])
    assert keep.sum() == 33
    pts, off, org = loop_cloud(d, s)
    assert same_bits(CR.points(d, s)[0], pts) and same_bits(CR.organized(d, s), org)


def test_restatement_equals_the_double_loop_on_random_maps():
    rng = np.random.default_rng(7)
    s = CR.spec(7, 5, fx=721.5377, fy=718.3, cx=3.1, cy=2.7, baseline=0.5327, doffs=0.37, frames=3, z_min=2.0, z_max=40.0, min_conf=20000)
    d = rng.uniform(-1, 64, (3, 5, 7)).astype(np.float32)
    d[rng.random(d.shape) < 0.2] = INF
    mask = (rng.random(d.shape) < 0.8).astype(np.uint8)
    conf = rng.integers(0, 65536, d.shape).astype(np.uint16)
    for m, k in ((None, None), (mask, None), (None, conf), (mask, conf)):
        pts, off, org = loop_cloud(d, s, m, k)
        got = CR.points(d, s, m, k)
        assert 0 < off[-1] < d.size
        assert same_bits(got[0], pts) and np.array_equal(got[1], off) and same_bits(CR.organized(d, s, m, k), org)


def test_z_of_kept_pixels_is_the_depth_conversion_on_the_cone_map():
    from soc_project_stereo_matching_amd import platform
    disp = load_npz("cone_final.npz")["final"]
    h, w = disp.shape
    fx, baseline, doffs = 1733.74, 536.62, 3.5
    s = CR.spec(w, h, fx=fx, fy=fx, cx=w / 2, cy=h / 2, baseline=baseline, doffs=doffs, z_min=20000.0, z_max=60000.0)
    keep, Z = CR.kept(disp, s)
    depth = platform.disparity_to_depth(disp, fx, baseline, doffs)
    assert 0.2 < keep.mean() < 0.9                                # z_min and z_max both cut into the data
    assert np.array_equal(Z[0][keep[0]].view(np.uint32), depth[keep[0]].view(np.uint32))
    pts, off = CR.points(disp, s)
    assert off[1] == keep.sum() and np.array_equal(pts["z"].view(np.uint32), depth[keep[0]].view(np.uint32))
    org = CR.organized(disp, s)
    assert np.all(org.view(np.uint32)[~keep] == CR.QNAN)


# ---- header, library, Python -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


NEW = ("sgm_cloud_organized", "sgm_cloud_points", "sgm_read_cloud", "SGM_ReadCloud", "sgm_rectify_valid_mask")


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    for name in ("sgmd_cloud_organized", "sgmd_cloud_points", "sgmd_cloud_scratch_bytes"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    for decl in (r"bool\s+sgm_cloud_organized\(sgm_instance\* s, const sgm_cloud_spec\* spec, const float\* d_disp, const uint8_t\* d_mask,\s*"
                 r"const uint16_t\* d_conf, float\* d_xyz\);",
                 r"bool\s+sgm_cloud_points\(sgm_instance\* s, const sgm_cloud_spec\* spec, const float\* d_disp, const uint8_t\* d_mask,\s*"
                 r"const uint16_t\* d_conf, sgm_point\* d_points, uint32_t\* d_offsets\);",
                 r"bool\s+sgm_read_cloud\(sgm_instance\* s, const sgm_cloud_spec\* spec, sgm_point\* points, size_t capacity, uint32_t\* offsets\);",
                 r"bool\s+sgm_rectify_valid_mask\(int width, int height, const float\* map_x, const float\* map_y, uint8_t\* mask\);",
                 r"typedef struct \{ float x, y, z; uint32_t pixel; \} sgm_point;"):
        assert re.search(decl, text), decl
    assert "X = (((float)x - cx) * Z) / fx" in text and "0x7FC00000" in text
    # the structs: 48 bytes of twelve 4-byte fields in the header's order; 16 bytes
    assert C.sizeof(S.SGMCloudSpec) == 48
    order = ["width", "height", "frames", "fx", "fy", "cx", "cy", "baseline", "doffs", "z_min", "z_max", "min_conf"]
    assert [f[0] for f in S.SGMCloudSpec._fields_] == order
    for k, name in enumerate(order):
        assert getattr(S.SGMCloudSpec, name).offset == 4 * k and getattr(S.SGMCloudSpec, name).size == 4, name
    body = re.search(r"typedef struct \{([^}]*)\} sgm_cloud_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == order
    assert S.POINT_DTYPE.itemsize == 16 and [S.POINT_DTYPE.fields[n][1] for n in ("x", "y", "z", "pixel")] == [0, 4, 8, 12]
    assert S.POINT_DTYPE == CR.POINT
    for m in ("cloud_organized", "cloud_points", "read_cloud"):
        assert callable(getattr(S.SGMInstance, m, None)), m
    assert callable(S.SGM.read_cloud) and callable(S.rectify_valid_mask) and callable(S.cloud_spec)
    sp = S.cloud_spec(7, 5, 1.0, 2.0, 3.0, 4.0, 5.0)
    assert (sp.frames, sp.z_min, sp.z_max, sp.min_conf, sp.doffs) == (1, 0.0, INF, 0, 0.0)


def test_driver_wants_a_pinhole_with_a_cloud(tmp_path):
    exe = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
    if not os.path.exists(exe):
        pytest.skip("sgm_main not built (no hipcc here)")
    # usage errors, told apart by what they say (an unknown option is exit status 2 as well)
    for extra, says in ((["--cloud", "c.ply"], "--cloud needs --pinhole"), (["--cloud", "c.ply", "--cloud-z-max", "9"], "--cloud needs --pinhole"),
                        (["--cloud", "c.ply", "--pinhole", "1,2,3"], "--pinhole wants FX,FY,CX,CY,BASELINE,DOFFS"),
                        (["--pinhole", "1,2,3,4,5,x", "--cloud", "c.ply"], "--pinhole wants FX,FY,CX,CY,BASELINE,DOFFS")):
        out = subprocess.run([exe, "a.png", "b.png", str(tmp_path / "o.png")] + extra, capture_output=True, text=True)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    # the options are known: with a pinhole the run gets as far as loading the images
    out = subprocess.run([exe, "a.png", "b.png", str(tmp_path / "o.png"), "--cloud", "c.ply", "--pinhole", "1,2,3,4,5,6", "--cloud-z-max", "9"],
                         capture_output=True, text=True)
    assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


# ---- host logic on the stand-in device -------------------------------------------------------------------------------------

class DeviceSpec(C.Structure):                                   # sgmd_cloud of csrc/sgm_device.h, as the stand-in logs it
    _fields_ = [("W", _i), ("H", _i), ("B", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "fb", "doffs", "z_min", "z_max")] + \
               [("min_conf", C.c_uint)]


def _sign(L):
    for name, (res, args) in {"sgm_cloud_organized": (_b, [_p] * 6), "sgm_cloud_points": (_b, [_p] * 7),
                              "sgm_read_cloud": (_b, [_p, _p, _p, _z, _p]), "SGM_ReadCloud": (_b, [_p, _p, _z, _p]),
                              "sgm_rectify_valid_mask": (_b, [_i, _i, _p, _p, _p]),
                              "SGM_Initialize": (_b, [C.c_uint16, C.c_uint16, _p]), "SGM_Match": (_b, [_p] * 3), "SGM_Shutdown": (None, []),
                              "stub_cloud_clear": (None, []), "stub_cloud_count": (_i, []), "stub_cloud_kind": (_i, [_i]),
                              "stub_cloud_ptr": (_p, [_i, _i]), "stub_cloud_spec": (C.POINTER(DeviceSpec), [_i]),
                              "stub_cloud_fail_at": (None, [_i]), "stub_fail_alloc_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("cloudstub"), extra_sources=[STUB_CLOUD], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("cloudstub_without"), flags=("-ffp-contract=off",)))


W, H = 48, 20


def c_spec(s):
    import soc_project_stereo_matching_amd as S
    return S.SGMCloudSpec(s.width, s.height, s.frames, s.fx, s.fy, s.cx, s.cy, s.baseline, s.doffs, s.z_min, s.z_max, s.min_conf)


def good_spec(w=W, h=H, frames=1, **kw):
    base = dict(fx=700.0, fy=710.0, cx=w / 2, cy=h / 2, baseline=160.0, doffs=0.75, frames=frames, z_min=100.0, z_max=1.0e6, min_conf=7)
    base.update(kw)
    return CR.spec(w, h, **base)


class Buffers:
    """a caller's "device" buffers on the stand-in: host memory"""
    def __init__(self, s, seed=3):
        rng = np.random.default_rng(seed)
        shape = (s.frames, s.height, s.width)
        self.disp = rng.uniform(-2, 64, shape).astype(np.float32)
        self.disp[rng.random(shape) < 0.2] = INF
        self.disp[rng.random(shape) < 0.02] = NAN
        self.mask = (rng.random(shape) < 0.8).astype(np.uint8)
        self.conf = rng.integers(0, 14, shape).astype(np.uint16)
        n = self.disp.size
        self.xyz = np.full((n, 3), -7, np.float32)
        self.points = np.zeros(n + 8, CR.POINT)
        self.points.view(np.uint8)[:] = 0xA5
        self.offsets = np.full(s.frames + 1, 0xA5A5A5A5, np.uint32)


def make(L, w=W, h=H, batch=1):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    opt = S.default_option(16)
    assert L.sgm_set_batch(s, batch) and L.sgm_reset(s, w, h, C.byref(opt))
    return s, opt


def test_device_forms_hand_the_validated_spec_and_the_callers_pointers_over(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: an explicit map needs no shape
    sp = good_spec(frames=2)
    b = Buffers(sp)
    cs = c_spec(sp)
    L.stub_clear(); L.stub_cloud_clear()
    assert L.sgm_cloud_organized(s, C.byref(cs), b.disp.ctypes.data, b.mask.ctypes.data, b.conf.ctypes.data, b.xyz.ctypes.data)
    assert L.sgm_cloud_points(s, C.byref(cs), b.disp.ctypes.data, None, b.conf.ctypes.data, b.points.ctypes.data, b.offsets.ctypes.data)
    assert L.stub_cloud_count() == 2 and (L.stub_cloud_kind(0), L.stub_cloud_kind(1)) == (0, 1)
    assert [L.stub_cloud_ptr(0, k) for k in range(4)] == [b.disp.ctypes.data, b.mask.ctypes.data, b.conf.ctypes.data, b.xyz.ctypes.data]
    assert [L.stub_cloud_ptr(1, k) for k in range(5)] == [b.disp.ctypes.data, None, b.conf.ctypes.data, b.points.ctypes.data,
                                                          b.offsets.ctypes.data]
    assert L.stub_cloud_ptr(1, 5) not in (None, b.points.ctypes.data)            # the instance's scratch
    d = L.stub_cloud_spec(1).contents
    assert (d.W, d.H, d.B, d.min_conf) == (W, H, 2, 7)
    assert np.float32(d.fb) == CR.fb_of(sp) and (d.fx, d.fy, d.doffs, d.z_min, d.z_max) == (700.0, 710.0, 0.75, 100.0, 1.0e6)
    # the stand-in computes for real: what arrived is the restatement
    assert same_bits(b.xyz.reshape(2, H, W, 3), CR.organized(b.disp, sp, b.mask, b.conf))
    want, off = CR.points(b.disp, sp, None, b.conf)
    assert np.array_equal(b.offsets, off) and same_bits(b.points[:off[-1]], want)
    assert np.all(b.points[off[-1]:].view(np.uint8) == 0xA5)
    # one allocation (the scratch) and nothing else on the device
    # (the first allocation of a buffer drains the instance's stream)
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", 0)]
    L.stub_clear()
    assert L.sgm_cloud_points(s, C.byref(cs), b.disp.ctypes.data, None, None, b.points.ctypes.data, b.offsets.ctypes.data)
    assert standin.launches(L, drop=()) == []                     # the scratch is kept
    L.sgm_destroy(s)


REFUSALS = {
    "width 0": dict(w=0), "width 65536": dict(w=65536), "height 0": dict(h=0), "height 65536": dict(h=65536), "frames 0": dict(frames=0),
    "frames -1": dict(frames=-1), "more than 2^31 pixels": dict(w=65535, h=65535), "2^31 + 1 pixel": dict(w=32769, h=65535),
    "fx 0": dict(fx=0.0), "fx < 0": dict(fx=-700.0), "fx NaN": dict(fx=NAN), "fx INF": dict(fx=INF), "fy 0": dict(fy=0.0), "fy NaN": dict(fy=NAN),
    "fy INF": dict(fy=INF), "baseline 0": dict(baseline=0.0), "baseline < 0": dict(baseline=-1.0), "baseline NaN": dict(baseline=NAN),
    "baseline INF": dict(baseline=INF), "fb overflows": dict(fx=3e20, baseline=3e20), "fb underflows to 0": dict(fx=1e-30, baseline=1e-30),
    "cx NaN": dict(cx=NAN), "cx INF": dict(cx=INF), "cy NaN": dict(cy=NAN), "cy -INF": dict(cy=-INF), "doffs NaN": dict(doffs=NAN),
    "doffs INF": dict(doffs=INF), "z_min NaN": dict(z_min=NAN), "z_min < 0": dict(z_min=-1.0), "z_max NaN": dict(z_max=NAN),
    "z_max == z_min": dict(z_min=5.0, z_max=5.0), "z_max < z_min": dict(z_min=5.0, z_max=4.0), "z_min INF": dict(z_min=INF, z_max=INF),
    "min_conf 65536": dict(min_conf=65536),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_false_and_queues_nothing(host, name):
    L = host
    s, _ = make(L)
    kw = dict(REFUSALS[name])
    sp = good_spec(kw.pop("w", W), kw.pop("h", H), **kw)
    cs = c_spec(sp)
    b = Buffers(good_spec())
    L.stub_clear(); L.stub_cloud_clear()
    assert not L.sgm_cloud_organized(s, C.byref(cs), b.disp.ctypes.data, None, None, b.xyz.ctypes.data)
    assert not L.sgm_cloud_points(s, C.byref(cs), b.disp.ctypes.data, None, None, b.points.ctypes.data, b.offsets.ctypes.data)
    assert not L.sgm_read_cloud(s, C.byref(cs), b.points.ctypes.data, b.points.size, b.offsets.ctypes.data)
    assert L.stub_cloud_count() == 0 and standin.log(L) == []
    L.sgm_destroy(s)


def test_null_arguments_and_the_accepted_edges(host):
    L = host
    s, _ = make(L)
    sp = good_spec()
    cs = c_spec(sp)
    b = Buffers(sp)
    d, x, p, o = b.disp.ctypes.data, b.xyz.ctypes.data, b.points.ctypes.data, b.offsets.ctypes.data
    L.stub_clear(); L.stub_cloud_clear()
    assert not L.sgm_cloud_organized(None, C.byref(cs), d, None, None, x) and not L.sgm_cloud_organized(s, None, d, None, None, x)
    assert not L.sgm_cloud_organized(s, C.byref(cs), d, None, None, None)
    assert not L.sgm_cloud_points(None, C.byref(cs), d, None, None, p, o) and not L.sgm_cloud_points(s, None, d, None, None, p, o)
    assert not L.sgm_cloud_points(s, C.byref(cs), d, None, None, None, o) and not L.sgm_cloud_points(s, C.byref(cs), d, None, None, p, None)
    assert not L.sgm_read_cloud(None, C.byref(cs), p, b.points.size, o) and not L.sgm_read_cloud(s, None, p, b.points.size, o)
    assert not L.sgm_read_cloud(s, C.byref(cs), p, b.points.size, None) and not L.sgm_read_cloud(s, C.byref(cs), None, 5, o)
    assert p % 16 == 0
    for skew in (4, 8, 12, 1):                                    # a list that is not 16-byte aligned
        assert not L.sgm_cloud_points(s, C.byref(cs), d, None, None, p + skew, o), skew
    assert L.stub_cloud_count() == 0 and standin.log(L) == []
    # allowed: z_min 0 with z_max +INF, min_conf 65535, doffs < 0, exactly 2^31 pixels is a spec the host accepts (not run here)
    for kw in (dict(z_min=0.0, z_max=INF), dict(min_conf=65535), dict(doffs=-3.0), dict(cx=-1e6, cy=1e6)):
        cs2 = c_spec(good_spec(**kw))
        assert L.sgm_cloud_organized(s, C.byref(cs2), d, None, None, x), kw
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_without, capfd):
    L = host_without
    s, opt = make(L)
    sp = good_spec()
    cs = c_spec(sp)
    b = Buffers(sp)
    left = np.zeros((H, W), np.uint8)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, b.disp.ctypes.data)
    capfd.readouterr()
    L.stub_clear()
    assert not L.sgm_cloud_organized(s, C.byref(cs), b.disp.ctypes.data, None, None, b.xyz.ctypes.data)
    assert "not part of this build" in capfd.readouterr().err
    assert not L.sgm_cloud_points(s, C.byref(cs), b.disp.ctypes.data, None, None, b.points.ctypes.data, b.offsets.ctypes.data)
    assert "not part of this build" in capfd.readouterr().err
    assert not L.sgm_read_cloud(s, C.byref(cs), b.points.ctypes.data, b.points.size, b.offsets.ctypes.data)
    assert "not part of this build" in capfd.readouterr().err
    assert standin.log(L) == []
    # the valid mask is host arithmetic: there in any build
    x, y = np.meshgrid(np.arange(4, dtype=np.float32), np.arange(3, dtype=np.float32))
    mask = np.full((3, 4), 9, np.uint8)
    assert L.sgm_rectify_valid_mask(4, 3, x.ctypes.data, y.ctypes.data, mask.ctypes.data) and mask.sum() == 6
    L.sgm_destroy(s)


def test_last_match_needs_the_instances_shape(host):
    L = host
    s, opt = make(L, batch=2)
    b = Buffers(good_spec(frames=2))
    left = np.zeros((2, H, W), np.uint8)
    out = np.zeros((2, H, W), np.float32)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    x, p, o = b.xyz.ctypes.data, b.points.ctypes.data, b.offsets.ctypes.data
    L.stub_clear(); L.stub_cloud_clear()
    for other in (good_spec(W + 1, H, frames=2), good_spec(W, H - 1, frames=2), good_spec(H, W, frames=2), good_spec(frames=1),
                  good_spec(frames=3)):
        cs = c_spec(other)
        assert not L.sgm_cloud_organized(s, C.byref(cs), None, None, None, x)
        assert not L.sgm_cloud_points(s, C.byref(cs), None, None, None, p, o)
        assert not L.sgm_read_cloud(s, C.byref(cs), p, b.points.size, o)
    assert L.stub_cloud_count() == 0 and standin.log(L) == []
    cs = c_spec(good_spec(frames=2))
    assert L.sgm_cloud_points(s, C.byref(cs), None, None, None, p, o) and L.stub_cloud_count() == 1
    inst_map = L.stub_cloud_ptr(0, 0)
    assert inst_map not in (None, out.ctypes.data)                # the instance's own final map
    # ... which is where stage 8 reads from
    L.stub_clear()
    got = np.zeros((H, W), np.float32)
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [inst_map]
    # after a match of both views the final left map lives elsewhere: the cloud follows stage 8
    assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_both(s, left.ctypes.data, left.ctypes.data, out.ctypes.data, b.disp.ctypes.data)
    L.stub_clear(); L.stub_cloud_clear()
    assert L.sgm_cloud_points(s, C.byref(cs), None, None, None, p, o)
    both_map = L.stub_cloud_ptr(0, 0)
    assert both_map != inst_map
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [both_map]
    # an instance that is not initialised has no last match; row tiles are refused
    assert L.sgm_set_rows(s, 4, 12)
    assert not L.sgm_cloud_points(s, C.byref(cs), None, None, None, p, o)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    assert not L.sgm_cloud_points(s, C.byref(cs), None, None, None, p, o)
    assert L.sgm_cloud_points(s, C.byref(cs), b.disp.ctypes.data, None, None, p, o)      # an explicit map still works
    assert L.sgm_set_rows(s, 0, 0)
    L.sgm_destroy(s)


def test_plain_match_logs_what_it_logs_without_the_clouds(host, host_without):
    """allocations and their sizes included: an instance that never asks for a cloud is the instance it was"""
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs, launches = [], []
    for L in (host, host_without):
        s = L.sgm_create(0)
        import soc_project_stereo_matching_amd as S
        opt = S.default_option(16)
        L.stub_clear()
        if hasattr(L, "stub_cloud_clear"):
            L.stub_cloud_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                                           conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        launches.append(standin.launches(L))
        L.sgm_destroy(s)
    assert launches[0] == launches[1] and logs[0] == logs[1]
    assert host.stub_cloud_count() == 0


def test_read_cloud_copies_offsets_then_exactly_the_records(host):
    L = host
    s, opt = make(L, batch=2)
    left = np.zeros((2, H, W), np.uint8)
    out = np.zeros((2, H, W), np.float32)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    sp = good_spec(frames=2)                                      # the stand-in's map is all 0: with doffs 0.75 every pixel is kept
    cs = c_spec(sp)
    n = 2 * W * H
    want, want_off = CR.points(np.zeros((2, H, W), np.float32), sp)
    assert want_off.tolist() == [0, W * H, n]
    pts = np.zeros(n + 4, CR.POINT)
    pts.view(np.uint8)[:] = 0xA5
    off = np.full(3, 0xA5A5A5A5, np.uint32)
    # too small: the offsets arrive, no record does
    L.stub_clear(); L.stub_cloud_clear()
    assert not L.sgm_read_cloud(s, C.byref(cs), pts.ctypes.data, n - 1, off.ctypes.data)
    assert np.array_equal(off, want_off) and np.all(pts.view(np.uint8) == 0xA5)
    copies = [e for e in standin.log(L) if e.name == "d2h"]
    assert [(e.arg, e.a) for e in copies] == [(12, off.ctypes.data)]
    assert L.stub_cloud_count() == 1 and L.stub_cloud_kind(0) == 1 and L.stub_cloud_ptr(0, 1) is None and L.stub_cloud_ptr(0, 2) is None
    # the device list is the instance's own buffer, not the caller's
    assert L.stub_cloud_ptr(0, 3) not in (None, pts.ctypes.data) and L.stub_cloud_ptr(0, 4) not in (None, off.ctypes.data)
    # NULL with capacity 0 asks for the size alone
    off[:] = 0
    assert not L.sgm_read_cloud(s, C.byref(cs), None, 0, off.ctypes.data) and off[2] == n
    # large enough: exactly `total` records
    L.stub_clear()
    assert L.sgm_read_cloud(s, C.byref(cs), pts.ctypes.data, n + 4, off.ctypes.data)
    copies = [e for e in standin.log(L) if e.name == "d2h"]
    assert [(e.arg, e.a) for e in copies] == [(12, off.ctypes.data), (16 * n, pts.ctypes.data)]
    assert same_bits(pts[:n], want) and np.all(pts[n:].view(np.uint8) == 0xA5)
    # nothing kept: true with no record copied
    cs0 = c_spec(good_spec(frames=2, z_max=101.0))
    L.stub_clear()
    assert L.sgm_read_cloud(s, C.byref(cs0), None, 0, off.ctypes.data) and off.tolist() == [0, 0, 0]
    assert len([e for e in standin.log(L) if e.name == "d2h"]) == 1
    L.sgm_destroy(s)


def test_read_cloud_of_the_default_instance_and_the_python_wrappers(host):
    import soc_project_stereo_matching_amd as S
    L = host
    opt = S.default_option(16)
    img = np.zeros((H, W), np.uint8)
    out = np.zeros((H, W), np.float32)
    sp = good_spec()
    cs = c_spec(sp)
    off = np.zeros(2, np.uint32)
    assert not L.SGM_ReadCloud(C.byref(cs), None, 0, off.ctypes.data)          # no default instance
    try:
        assert L.SGM_Initialize(W, H, C.byref(opt)) and L.SGM_Match(img.ctypes.data, img.ctypes.data, out.ctypes.data)
        # the wrapper's two-call protocol, on the stand-in's library
        from soc_project_stereo_matching_amd.sgm import _read_cloud
        got = _read_cloud(L.SGM_ReadCloud, cs)
        want = CR.points(np.zeros((1, H, W), np.float32), sp)
        assert got is not None and same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
        empty = _read_cloud(L.SGM_ReadCloud, c_spec(good_spec(z_max=101.0)))
        assert empty is not None and empty[0].size == 0 and empty[1].tolist() == [0, 0]
        assert _read_cloud(L.SGM_ReadCloud, c_spec(good_spec(fx=0.0))) is None
    finally:
        L.SGM_Shutdown()


def test_a_refused_launch_or_allocation_fails_the_call(host):
    L = host
    s, opt = make(L)
    sp = good_spec()
    cs = c_spec(sp)
    b = Buffers(sp)
    left = np.zeros((H, W), np.uint8)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, b.xyz.ctypes.data)
    d, x, p, o = b.disp.ctypes.data, b.xyz.ctypes.data, b.points.ctypes.data, b.offsets.ctypes.data
    calls = {"organized": lambda: L.sgm_cloud_organized(s, C.byref(cs), d, None, None, x),
             "points": lambda: L.sgm_cloud_points(s, C.byref(cs), d, None, None, p, o),
             "read": lambda: L.sgm_read_cloud(s, C.byref(cs), p, b.points.size, o)}
    for name, call in calls.items():
        L.stub_cloud_clear()
        L.stub_cloud_fail_at(0)
        assert not call(), name
        assert call(), name                                       # and the instance goes on
    # with the post pass on a stream of its own the cloud waits for the result of a match that is still in flight
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    for name, call in calls.items():
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, b.xyz.ctypes.data)
        L.stub_clear()
        assert call(), name
        assert "wait_event" in [e.name for e in standin.log(L)], name
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, b.xyz.ctypes.data)    # (the blocking form drained it)
        L.stub_clear()
        L.stub_fail_at(b"wait_event", 0)
        L.stub_cloud_clear()
        assert not call() and L.stub_cloud_count() == 0, name
    L.sgm_destroy(s)
    # every allocation of a first sgm_read_cloud, refused in turn
    for k in range(3):
        s, opt = make(L)
        assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, b.xyz.ctypes.data)
        L.stub_fail_alloc_at(k)
        ok = L.sgm_read_cloud(s, C.byref(cs), p, b.points.size, o)
        L.stub_fail_alloc_at(-1)
        assert not ok, k
        assert L.sgm_read_cloud(s, C.byref(cs), p, b.points.size, o), k
        L.sgm_destroy(s)


# ---- sgm_rectify_valid_mask --------------------------------------------------------------------------------------------------

def ref_valid_mask(mx, my):
    """all four taps of rectify_ref.remap_q inside the frame"""
    h, w = mx.shape
    xq, yq = RR.quantise(mx, my)
    x0, y0 = xq.astype(np.int64) >> 5, yq.astype(np.int64) >> 5
    return ((x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)).astype(np.uint8)


@pytest.mark.parametrize("w,h", [(70, 33), (20, 31), (33, 33)])
def test_valid_mask_equals_the_rectification_restatement(lib, w, h):
    import soc_project_stereo_matching_amd as S
    from test_gpu_rectify import kernel_maps
    maps = kernel_maps(w, h)
    for name in ("identity", "shift", "rotation30", "radial", "outside", "sprinkled", "weights"):
        mx, my = (np.ascontiguousarray(m, np.float32) for m in maps[name])
        got = S.rectify_valid_mask(mx, my)
        want = ref_valid_mask(mx, my)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        white = RR.remap(np.full((h, w), 255, np.uint8), mx, my)
        assert np.all(white[got == 1] == 255), name
        if name == "outside":
            assert not got.any()
        if name == "identity":
            assert got[:-1, :-1].all() and not got[-1].any() and not got[:, -1].any()
        if name in ("rotation30", "radial", "sprinkled"):
            assert 0 < got.sum() < w * h, name


def test_valid_mask_edges_and_refusals(lib):
    import soc_project_stereo_matching_amd as S
    w, h = 8, 4
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    for v in (np.nan, np.inf, -np.inf, 1e9, 32768.5, -40000.0):
        mx = x.copy()
        mx[1, 2] = v
        assert S.rectify_valid_mask(mx, y)[1, 2] == 0 and S.rectify_valid_mask(y * 0 + 1, mx)[1, 2] == 0
    mx = x.copy()
    mx[0, 0] = -1 / 64                                           # rounds to xq = 0 (floor(-0.5 + 0.5)): still inside
    mx[0, 1] = -1 / 32                                           # xq = -1: the left taps are outside
    mx[0, 2] = w - 2 + 31 / 32                                   # the last position with both columns inside
    mx[0, 3] = w - 2 + 63 / 64                                   # rounds up to x0 = w - 1
    assert S.rectify_valid_mask(mx, y)[0, :4].tolist() == [1, 0, 1, 0]
    assert np.array_equal(S.rectify_valid_mask(mx, y), ref_valid_mask(mx, y))
    one = np.zeros((1, 1), np.float32)
    assert S.rectify_valid_mask(one, one)[0, 0] == 0              # a 1x1 image has no four taps
    f = lib.sgm_rectify_valid_mask
    out = np.zeros((h, w), np.uint8)
    assert f(w, h, x.ctypes.data, y.ctypes.data, out.ctypes.data)
    for bad in ((0, h), (w, 0), (-1, h)):
        assert not f(*bad, x.ctypes.data, y.ctypes.data, out.ctypes.data)
    assert not f(w, h, None, y.ctypes.data, out.ctypes.data) and not f(w, h, x.ctypes.data, None, out.ctypes.data)
    assert not f(w, h, x.ctypes.data, y.ctypes.data, None)
    with pytest.raises(ValueError):
        S.rectify_valid_mask(x, y[:2])


# ---- sanitizers on a stand-alone program -----------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_cloud_host_is_asan_ubsan_clean(tmp_path):
    """tests/cloud_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in clouds."""
    exe = standin.build(tmp_path, sanitize=True, exe="cloud_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "cloud_sanitize_driver.c"), STUB_CLOUD])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("cloud_sanitize_driver ok")
