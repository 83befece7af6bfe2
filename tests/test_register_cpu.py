"""Depth registered to another camera (extension; the contract is in include/sgm_mi355x.h, sgm_register_spec) without a GPU: the
numpy restatement tests/register_ref.py against a plain-Python loop, against the cloud (identity) and against the rectification's
maps (the raw camera); header / library / Python agreement; the C host's logic on the stand-in device (tests/stub_device.c +
tests/stub_register.c); and a sanitizer run of a stand-alone driver.  Tolerance 0 everywhere."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import rectify_ref as RR
import register_ref as GR
import standin
from conftest import ROOT
from test_cloud_cpu import f32, div32, same_bits

STUB_REGISTER = os.path.join(ROOT, "tests", "stub_register.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
INF, NAN = float("inf"), float("nan")


def ramp_block(w, h, frames, seed=0):
    """a ramp across the frame with a nearer block in front of it, an invalid patch and a frame-dependent offset"""
    x = np.arange(w, dtype=np.float32)[None, None, :]
    y = np.arange(h, dtype=np.float32)[None, :, None]
    f = np.arange(frames, dtype=np.float32)[:, None, None]
    d = (np.float32(6) + x * np.float32(0.25) + y * np.float32(0.125) + f).astype(np.float32)
    d[:, h // 4:h // 2, w // 3:w // 2] = np.float32(48.5)
    d[:, h - 3:, :5] = np.inf
    return np.ascontiguousarray(np.broadcast_to(d, (frames, h, w)))


def source_spec(w, h, frames=1, **kw):
    base = dict(fx=721.5377, fy=718.856, cx=w / 2 - 0.37, cy=h / 2 + 0.21, baseline=0.54, doffs=0.25, frames=frames)
    base.update(kw)
    return CR.spec(w, h, **base)


# ---- the restatement against a plain-Python loop -----------------------------------------------------------------------------

def loop_register(disp, s, r, mask=None, conf=None):
    """The definition of include/sgm_mi355x.h as a loop over Python floats, every operation rounded to float32 once (sums,
    products and quotients of two float32 values are exact or correctly rounded in double)."""
    fb = f32(float(np.float32(s.fx)) * float(np.float32(s.baseline)))
    fx, fy, cx, cy, doffs, z_min, z_max = (float(np.float32(v)) for v in (s.fx, s.fy, s.cx, s.cy, s.doffs, s.z_min, s.z_max))
    R, t = [float(np.float32(v)) for v in r.R], [float(np.float32(v)) for v in r.t]
    k1, k2, p1, p2, k3 = (float(np.float32(v)) for v in r.dist)
    tfx, tfy, tcx, tcy, tz_min, tz_max = (float(np.float32(v)) for v in (r.fx, r.fy, r.cx, r.cy, r.z_min, r.z_max))
    w, h = r.width, r.height
    best = {}

    def mad(a, x, b, y):
        return f32(f32(a * x) + f32(b * y))

    for f in range(s.frames):
        for y in range(s.height):
            for x in range(s.width):
                d = float(disp[f, y, x])
                if not math.isfinite(d) or (mask is not None and mask[f, y, x] == 0) or (conf is not None and int(conf[f, y, x]) < s.min_conf):
                    continue
                den = f32(d + doffs)
                if not math.isfinite(den) or not den > 0:
                    continue
                Z = div32(fb, den)
                if not math.isfinite(Z) or not (z_min <= Z <= z_max):
                    continue
                X = div32(f32(f32(x - cx) * Z), fx)
                Y = div32(f32(f32(y - cy) * Z), fy)
                P = [f32(f32(mad(R[3 * i], X, R[3 * i + 1], Y) + f32(R[3 * i + 2] * Z)) + t[i]) for i in range(3)]
                Zp = P[2]
                if not math.isfinite(Zp) or not (Zp > 0 and tz_min <= Zp <= tz_max):
                    continue
                a, b = div32(P[0], Zp), div32(P[1], Zp)
                if not (math.isfinite(a) and math.isfinite(b)):
                    continue                                      # (then u or v is not finite either)
                aa, bb, ab = f32(a * a), f32(b * b), f32(a * b)
                r2 = f32(aa + bb)
                rad = f32(f32(f32(f32(f32(f32(k3 * r2) + k2) * r2) + k1) * r2) + 1.0)
                xd = f32(f32(f32(a * rad) + f32(f32(2.0 * p1) * ab)) + f32(p2 * f32(r2 + f32(2.0 * aa))))
                yd = f32(f32(f32(b * rad) + f32(p1 * f32(r2 + f32(2.0 * bb)))) + f32(f32(2.0 * p2) * ab))
                u, v = f32(f32(tfx * xd) + tcx), f32(f32(tfy * yd) + tcy)
                if not (math.isfinite(u) and math.isfinite(v)):
                    continue
                if r.splat == 1:
                    cands = [(math.floor(f32(u + 0.5)), math.floor(f32(v + 0.5)))]
                else:
                    u0, v0 = math.floor(u), math.floor(v)
                    cands = [(u0, v0), (u0 + 1, v0), (u0, v0 + 1), (u0 + 1, v0 + 1)]
                key = (int(np.float32(Zp).view(np.uint32)) << 32) | (y << 16) | x
                for uf, vf in cands:
                    if 0 <= uf < w and 0 <= vf < h:
                        at = (f, int(vf), int(uf))
                        best[at] = min(best.get(at, 1 << 64), key)
    depth = np.full((s.frames, h, w), GR.QNAN, np.uint32)
    source = np.full((s.frames, h, w), GR.NONE, np.uint32)
    for at, key in best.items():
        depth[at], source[at] = key >> 32, key & 0xFFFFFFFF
    return depth.view(np.float32), source


def colour_camera(w=13, h=9, splat=2, **kw):
    """a second camera beside the pair: a small rotation, a shift, all five distortion coefficients"""
    a, b = np.deg2rad(2.0), np.deg2rad(-1.5)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    base = dict(fx=0.75 * 721.5377 * w / 13, fy=0.75 * 718.856 * w / 13, cx=w / 2 + 0.2, cy=h / 2 - 0.3, dist=(-0.08, 0.02, 0.001, -0.001, 0.003),
                R=Rz @ Ry, t=(0.05, -0.01, 0.002), splat=splat)
    base.update(kw)
    return GR.spec(w, h, **base)


@pytest.mark.parametrize("splat", [1, 2])
def test_restatement_equals_the_loop(splat):
    rng = np.random.default_rng(7 + splat)
    s = source_spec(17, 11, frames=2, z_min=2.0, z_max=80.0, min_conf=20000)
    d = rng.uniform(-1, 64, (2, 11, 17)).astype(np.float32)
    d[rng.random(d.shape) < 0.1] = INF
    d[0, 0, :3] = (NAN, -INF, 0.0)
    mask = (rng.random(d.shape) < 0.8).astype(np.uint8)
    conf = rng.integers(0, 65536, d.shape).astype(np.uint16)
    targets = {"colour": colour_camera(13, 9, splat, fx=260.0, fy=258.0), "identity": GR.spec(17, 11, s.fx, s.fy, s.cx, s.cy, splat=splat),
               "one pixel": GR.spec(1, 1, 1e-3, 1e-3, 0.4, 0.4, splat=splat),
               "cut in depth": colour_camera(13, 9, splat, fx=260.0, fy=258.0, z_min=6.0, z_max=30.0),
               "behind the camera": GR.spec(9, 9, 100.0, 100.0, 4.0, 4.0, R=(1, 0, 0, 0, -1, 0, 0, 0, -1), splat=splat)}
    for name, r in targets.items():
        for m, k in ((None, None), (mask, conf)):
            want_d, want_s = loop_register(d, s, r, m, k)
            got_d, got_s = GR.register(d, s, r, m, k)
            assert same_bits(got_d, want_d) and same_bits(got_s, want_s), name
            hit = got_s != GR.NONE
            if name == "behind the camera":
                assert not hit.any()
            else:
                assert hit.any(), name
            assert np.all(got_d.view(np.uint32)[~hit] == GR.QNAN)
    assert (GR.register(d, s, targets["one pixel"])[1] != GR.NONE).all()


def test_identity_returns_every_kept_pixel_to_itself():
    """same pinhole, R = I, t = 0, no distortion, splat 1: source == the pixel's own index and depth == the cloud's Z bit for bit on
    every kept pixel, NaN elsewhere"""
    w, h, frames = 70, 33, 3
    s = source_spec(w, h, frames)
    d = ramp_block(w, h, frames)
    keep, Z = CR.kept(d, s)
    assert 0.9 < keep.mean() < 1.0
    depth, source = GR.register(d, s, GR.spec(w, h, s.fx, s.fy, s.cx, s.cy, splat=1))
    own = np.broadcast_to((np.arange(h, dtype=np.uint32)[:, None] << np.uint32(16)) | np.arange(w, dtype=np.uint32)[None, :], keep.shape)
    assert np.array_equal(source[keep], own[keep]) and np.all(source[~keep] == GR.NONE)
    assert np.array_equal(depth.view(np.uint32)[keep], Z.view(np.uint32)[keep]) and np.all(depth.view(np.uint32)[~keep] == GR.QNAN)
    # ... and the organised cloud's Z, which is the same array
    assert np.array_equal(depth.view(np.uint32)[keep], CR.organized(d, s).view(np.uint32)[..., 2][keep])


MODELS = {"PLAIN": RR.PLAIN, "SMALL": RR.SMALL, "ROTATED": RR.ROTATED, "RADIAL": RR.RADIAL}


@pytest.mark.parametrize("w,h", [(37, 21), (70, 33), (256, 130)])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_raw_camera_target_agrees_with_the_rectification_maps(model, w, h):
    """sgm_rectify_maps says where in the raw image a rectified pixel comes from; registering into register_spec_raw's camera must
    send the pixel back there whatever its depth.  Checked: every source pixel whose map value rounds inside the frame, lies more
    than 1/1000 px from a rounding boundary and is the only one expected at its target.  The boundary exclusion leaves out at most
    1 % of the in-frame pixels."""
    K, dist, R, Knew = RR.model(MODELS[model], w, h)
    mx, my = (np.asarray(m, np.float64) for m in RR.maps(K, dist, R, Knew, w, h))
    s = CR.spec(w, h, fx=Knew[0, 0], fy=Knew[1, 1], cx=Knew[0, 2], cy=Knew[1, 2], baseline=0.54)
    r = GR.spec_raw(K, dist, R, w, h, splat=1)
    d = np.random.default_rng(w + h).uniform(4, 60, (1, h, w)).astype(np.float32)
    _, source = GR.register(d, s, r)
    eps = 1e-3
    # the targets a pixel may reach when its projection is off by up to eps either way
    reach = [(np.floor(mx + 0.5 + dx), np.floor(my + 0.5 + dy)) for dx in (-eps, eps) for dy in (-eps, eps)]
    tx, ty = np.floor(mx + 0.5), np.floor(my + 0.5)
    in_frame = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    sure = np.all([(ax == tx) & (ay == ty) for ax, ay in reach], axis=0)
    expected = np.zeros((h, w), np.int64)                        # how many source pixels may reach a target
    for k, (ax, ay) in enumerate(reach):
        ok = (ax >= 0) & (ax < w) & (ay >= 0) & (ay < h)
        for prev_x, prev_y in reach[:k]:                         # a pixel counts once per distinct target
            ok &= ~((prev_x == ax) & (prev_y == ay))
        np.add.at(expected, (ay[ok].astype(np.int64), ax[ok].astype(np.int64)), 1)
    txi, tyi = np.where(in_frame, tx, 0).astype(np.int64), np.where(in_frame, ty, 0).astype(np.int64)
    check = in_frame & sure & (expected[tyi, txi] == 1)
    left_out = (in_frame & ~sure).sum() / max(int(in_frame.sum()), 1)
    assert in_frame.sum() > 0.3 * w * h and check.sum() > 0.1 * w * h, (model, in_frame.sum(), check.sum())
    assert left_out <= 0.01, (model, w, h, left_out)
    own = (np.arange(h, dtype=np.uint32)[:, None] << np.uint32(16)) | np.arange(w, dtype=np.uint32)[None, :]
    got = source[0][tyi[check], txi[check]]
    assert np.array_equal(got, own[check]), (model, w, h, int((got != own[check]).sum()), int(check.sum()))


# ---- header, library, Python -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


FIELDS = ["width", "height", "fx", "fy", "cx", "cy", "dist", "R", "t", "z_min", "z_max", "splat"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 44, 80, 92, 96, 100]


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in ("sgm_register_depth", "sgm_register_gather", "sgm_register_spec_raw"):
        assert name in declared and hasattr(lib, name), name
    for name in ("sgmd_register_depth", "sgmd_register_gather", "sgmd_register_scratch_bytes"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    for decl in (r"bool\s+sgm_register_depth\(sgm_instance\* s, const sgm_cloud_spec\* src, const sgm_register_spec\* dst,\s*"
                 r"const float\* d_disp, const uint8_t\* d_mask, const uint16_t\* d_conf,\s*float\* d_depth, uint32_t\* d_source",
                 r"bool\s+sgm_register_gather\(sgm_instance\* s, const sgm_cloud_spec\* src, const sgm_register_spec\* dst,\s*"
                 r"const uint32_t\* d_source, int elem_bytes[^\n]*,\s*const void\* d_map, const void\* fill, void\* d_out\);",
                 r"bool\s+sgm_register_spec_raw\(const double K\[9\], const double dist\[5\], const double R\[9\],\s*"
                 r"int width, int height, int splat, sgm_register_spec\* out\);"):
        assert re.search(decl, text), decl
    assert "X' = ((R0*X + R1*Y) + R2*Z) + t0" in text and "rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1" in text
    assert C.sizeof(S.SGMRegisterSpec) == 104
    assert [f[0] for f in S.SGMRegisterSpec._fields_] == FIELDS
    assert [getattr(S.SGMRegisterSpec, n).offset for n in FIELDS] == OFFSETS
    body = re.search(r"typedef struct \{([^}]*)\} sgm_register_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == FIELDS
    for m in ("register_depth", "register_gather"):
        assert callable(getattr(S.SGMInstance, m, None)), m
    sp = S.register_spec(7, 5, 1.0, 2.0, 3.0, 4.0)
    assert (sp.z_min, sp.z_max, sp.splat, list(sp.R), list(sp.t), list(sp.dist)) == (0.0, INF, 2, list(GR.IDENTITY), [0.0] * 3, [0.0] * 5)
    assert S.REGISTER_NONE == int(GR.NONE)


def c_target(r):
    import soc_project_stereo_matching_amd as S
    return S.register_spec(r.width, r.height, r.fx, r.fy, r.cx, r.cy, r.dist, r.R, r.t, r.z_min, r.z_max, r.splat)


def test_spec_raw_is_the_transpose_rounded_once(lib):
    import soc_project_stereo_matching_amd as S
    K, dist, R, _ = RR.model(RR.SMALL, 70, 33)
    got = S.register_spec_raw(K, dist, R, 70, 33, 1)
    want = c_target(GR.spec_raw(K, dist, R, 70, 33, 1))
    assert bytes(got) == bytes(want)
    assert list(got.R) == [float(np.float32(v)) for v in np.asarray(R).T.reshape(9)] and list(got.t) == [0.0] * 3
    assert (got.z_min, got.z_max, got.splat, got.width, got.height) == (0.0, INF, 1, 70, 33)
    out = S.SGMRegisterSpec()
    k, d, r = (np.ascontiguousarray(m, np.float64).reshape(-1) for m in (K, dist, R))
    f = lib.sgm_register_spec_raw
    assert f(k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 33, 2, C.byref(out))
    for args in ((None, d.ctypes.data, r.ctypes.data, 70, 33, 2, C.byref(out)), (k.ctypes.data, None, r.ctypes.data, 70, 33, 2, C.byref(out)),
                 (k.ctypes.data, d.ctypes.data, None, 70, 33, 2, C.byref(out)), (k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 33, 2, None),
                 (k.ctypes.data, d.ctypes.data, r.ctypes.data, 0, 33, 2, C.byref(out)), (k.ctypes.data, d.ctypes.data, r.ctypes.data, 65536, 33, 2, C.byref(out)),
                 (k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 0, 2, C.byref(out)), (k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 65536, 2, C.byref(out)),
                 (k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 33, 0, C.byref(out)), (k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 33, 3, C.byref(out))):
        assert not f(*args), args
    for arr in (k, d, r):
        for bad in (NAN, INF):
            keep = arr[1]
            arr[1] = bad
            assert not f(k.ctypes.data, d.ctypes.data, r.ctypes.data, 70, 33, 2, C.byref(out))
            arr[1] = keep
    assert f(k.ctypes.data, d.ctypes.data, r.ctypes.data, 65535, 1, 1, C.byref(out))


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

class DeviceSrc(C.Structure):                                    # sgmd_cloud of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i), ("B", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "fb", "doffs", "z_min", "z_max")] + \
               [("min_conf", C.c_uint)]


class DeviceDst(C.Structure):                                    # sgmd_register of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] + \
               [("dist", C.c_float * 5), ("R", C.c_float * 9), ("t", C.c_float * 3), ("z_min", C.c_float), ("z_max", C.c_float), ("splat", _i)]


def _sign(L):
    for name, (res, args) in {"sgm_register_depth": (_b, [_p] * 8), "sgm_register_gather": (_b, [_p] * 4 + [_i] + [_p] * 3),
                              "stub_register_clear": (None, []), "stub_register_count": (_i, []), "stub_register_kind": (_i, [_i]),
                              "stub_register_ptr": (_p, [_i, _i]), "stub_register_src": (C.POINTER(DeviceSrc), [_i]),
                              "stub_register_dst": (C.POINTER(DeviceDst), [_i]), "stub_register_elem": (_i, [_i]),
                              "stub_register_fill": (C.c_uint, [_i]), "stub_register_fail_at": (None, [_i]),
                              "stub_fail_alloc_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("registerstub"), extra_sources=[STUB_REGISTER], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("registerstub_without"), flags=("-ffp-contract=off",)))


W, H = 48, 20


def c_source(s):
    import soc_project_stereo_matching_amd as S
    return S.SGMCloudSpec(s.width, s.height, s.frames, s.fx, s.fy, s.cx, s.cy, s.baseline, s.doffs, s.z_min, s.z_max, s.min_conf)


class Buffers:
    """a caller's "device" buffers on the stand-in: host memory, the outputs pre-filled with 0xA5"""
    def __init__(self, s, r, seed=3):
        rng = np.random.default_rng(seed)
        shape = (s.frames, s.height, s.width)
        self.disp = rng.uniform(2, 64, shape).astype(np.float32)
        self.disp[rng.random(shape) < 0.2] = INF
        self.disp[rng.random(shape) < 0.02] = NAN
        self.mask = (rng.random(shape) < 0.8).astype(np.uint8)
        self.conf = rng.integers(0, 14, shape).astype(np.uint16)
        n = s.frames * r.height * r.width
        self.depth = np.full(n + 4, 0xA5, np.uint8).repeat(4).view(np.uint32)
        self.source = self.depth.copy()
        self.n = n

    def untouched(self):
        return bool(np.all(self.depth == 0xA5A5A5A5) and np.all(self.source == 0xA5A5A5A5))


def make(L, w=W, h=H, batch=1):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    opt = S.default_option(16)
    assert L.sgm_set_batch(s, batch) and L.sgm_reset(s, w, h, C.byref(opt))
    return s, opt


def good_source(frames=1, **kw):
    return source_spec(W, H, frames, min_conf=7, **kw)


def good_target(w=31, h=17, **kw):
    return colour_camera(w, h, **kw)


def depth_call(L, s, cs, ct, b, disp="own", mask=None, conf=None, depth="own", source="own"):
    return L.sgm_register_depth(s, None if cs is None else C.byref(cs), None if ct is None else C.byref(ct),
                                b.disp.ctypes.data if isinstance(disp, str) else disp, mask, conf,
                                b.depth.ctypes.data if isinstance(depth, str) else depth,
                                b.source.ctypes.data if isinstance(source, str) else source)


def test_the_validated_specs_and_the_callers_pointers_arrive(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: an explicit map needs no shape
    sp, tg = good_source(frames=2), good_target()
    b = Buffers(sp, tg)
    cs, ct = c_source(sp), c_target(tg)
    L.stub_clear(); L.stub_register_clear()
    assert depth_call(L, s, cs, ct, b, mask=b.mask.ctypes.data, conf=b.conf.ctypes.data)
    assert L.stub_register_count() == 1 and L.stub_register_kind(0) == 0
    assert [L.stub_register_ptr(0, k) for k in (0, 1, 2, 4, 5)] == [b.disp.ctypes.data, b.mask.ctypes.data, b.conf.ctypes.data,
                                                                    b.depth.ctypes.data, b.source.ctypes.data]
    keys = L.stub_register_ptr(0, 3)
    assert keys not in (None, b.depth.ctypes.data) and keys % 16 == 0
    d, t = L.stub_register_src(0).contents, L.stub_register_dst(0).contents
    assert (d.W, d.H, d.B, d.min_conf) == (W, H, 2, 7) and np.float32(d.fb) == CR.fb_of(sp)
    assert bytes(t)[8:] == bytes(ct)[8:] and (t.W, t.H, t.splat) == (31, 17, 2)
    # the stand-in computes for real: what arrived is the restatement
    want_d, want_s = GR.register(b.disp, sp, tg, b.mask, b.conf)
    assert (want_s != GR.NONE).sum() > 50
    assert same_bits(b.depth[:b.n].view(np.float32).reshape(want_d.shape), want_d) and same_bits(b.source[:b.n].reshape(want_s.shape), want_s)
    assert np.all(b.depth[b.n:] == 0xA5A5A5A5) and np.all(b.source[b.n:] == 0xA5A5A5A5)
    # one allocation (the keys: the first allocation of a buffer drains the instance's stream) and nothing else on the device
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", (2 * 31 * 17 * 8) >> 10)]     # 8 bytes per target pixel, logged in KiB
    # the keys are kept: the same call again, and a smaller target, allocate nothing; d_source may be NULL
    L.stub_clear()
    assert depth_call(L, s, cs, ct, b, source=None) and L.stub_register_ptr(1, 5) is None
    small = good_target(9, 5)
    assert depth_call(L, s, cs, c_target(small), b)
    assert standin.launches(L, drop=()) == [] and L.stub_register_ptr(2, 3) == keys
    want_d, want_s = GR.register(b.disp, sp, small)
    assert same_bits(b.depth[:2 * 45].view(np.float32).reshape(want_d.shape), want_d) and same_bits(b.source[:2 * 45].reshape(want_s.shape), want_s)
    # a larger one grows them: a drain and an allocation of the new size
    big = good_target(64, 40)
    b2 = Buffers(sp, big)
    L.stub_clear()
    assert depth_call(L, s, cs, c_target(big), b2)
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", (2 * 64 * 40 * 8) >> 10)]
    want_d, want_s = GR.register(b2.disp, sp, big)
    assert same_bits(b2.depth[:b2.n].view(np.float32).reshape(want_d.shape), want_d) and same_bits(b2.source[:b2.n].reshape(want_s.shape), want_s)
    L.sgm_destroy(s)


def test_gather_hands_over_the_element_and_the_fill(host):
    L = host
    s = L.sgm_create(0)
    sp, tg = good_source(frames=2), good_target()
    b = Buffers(sp, tg)
    cs, ct = c_source(sp), c_target(tg)
    assert depth_call(L, s, cs, ct, b)
    source = b.source[:b.n].reshape(2, tg.height, tg.width)
    rng = np.random.default_rng(5)
    L.stub_clear(); L.stub_register_clear()
    for k, (dtype, fill) in enumerate(((np.uint8, 0xEE), (np.uint16, 0xBEEF), (np.float32, -7.5))):
        values = (rng.random((2, H, W)) * 200).astype(dtype)
        out = np.full(b.n + 4, 0xA5, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype)
        fv = np.array([fill], dtype)
        assert L.sgm_register_gather(s, C.byref(cs), C.byref(ct), b.source.ctypes.data, fv.itemsize, values.ctypes.data, fv.ctypes.data,
                                     out.ctypes.data)
        assert L.stub_register_kind(k) == 1 and L.stub_register_elem(k) == fv.itemsize
        assert L.stub_register_fill(k) == int(fv.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[fv.itemsize])[0])
        assert [L.stub_register_ptr(k, j) for j in range(3)] == [b.source.ctypes.data, values.ctypes.data, out.ctypes.data]
        assert same_bits(out[:b.n].reshape(source.shape), GR.gather(source, values, fv[0]))
        assert np.all(out[b.n:].view(np.uint8) == 0xA5)
    assert standin.log(L) == []                                   # no allocation, no copy
    L.sgm_destroy(s)


_T = dict  # shorthand below
SOURCE_REFUSALS = {
    "src width 0": _T(w=0), "src width 65536": _T(w=65536), "src height 0": _T(h=0), "src frames 0": _T(frames=0),
    "src more than 2^31 pixels": _T(w=65535, h=65535), "src fx 0": _T(fx=0.0), "src fy NaN": _T(fy=NAN), "src baseline 0": _T(baseline=0.0),
    "src cx INF": _T(cx=INF), "src doffs NaN": _T(doffs=NAN), "src z_min < 0": _T(z_min=-1.0), "src z_max == z_min": _T(z_min=5.0, z_max=5.0),
    "src min_conf 65536": _T(min_conf=65536),
}
R_BAD = list(GR.IDENTITY)
R_BAD[5] = NAN
TARGET_REFUSALS = {
    "width 0": _T(w=0), "width -1": _T(w=-1), "width 65536": _T(w=65536), "height 0": _T(h=0), "height 65536": _T(h=65536),
    "frames * width * height > 2^31": _T(w=65535, h=65535), "fx 0": _T(fx=0.0), "fx < 0": _T(fx=-5.0), "fx NaN": _T(fx=NAN), "fx INF": _T(fx=INF),
    "fy 0": _T(fy=0.0), "fy NaN": _T(fy=NAN), "fy INF": _T(fy=INF), "cx NaN": _T(cx=NAN), "cx INF": _T(cx=INF), "cy NaN": _T(cy=NAN),
    "cy -INF": _T(cy=-INF), "dist NaN": _T(dist=(0, 0, NAN, 0, 0)), "dist INF": _T(dist=(INF, 0, 0, 0, 0)), "k3 -INF": _T(dist=(0, 0, 0, 0, -INF)),
    "R NaN": _T(R=R_BAD), "R INF": _T(R=[INF] + list(GR.IDENTITY[1:])), "t NaN": _T(t=(0, NAN, 0)), "t INF": _T(t=(0, 0, INF)),
    "z_min NaN": _T(z_min=NAN), "z_min < 0": _T(z_min=-1.0), "z_max NaN": _T(z_max=NAN), "z_max == z_min": _T(z_min=5.0, z_max=5.0),
    "z_max < z_min": _T(z_min=5.0, z_max=4.0), "z_min INF": _T(z_min=INF, z_max=INF), "splat 0": _T(splat=0), "splat 3": _T(splat=3),
    "splat 4": _T(splat=4), "splat -1": _T(splat=-1),
}


def _refused(L, s, cs, ct, b, capfd):
    """both entry points answer false with a message, queue nothing and leave the outputs alone"""
    fv = np.zeros(1, np.uint16)
    values = np.zeros((1, H, W), np.uint16)
    L.stub_clear(); L.stub_register_clear()
    capfd.readouterr()
    assert not depth_call(L, s, cs, ct, b)
    assert "sgm_mi355x:" in capfd.readouterr().err
    assert not L.sgm_register_gather(s, C.byref(cs), C.byref(ct), b.source.ctypes.data, 2, values.ctypes.data, fv.ctypes.data, b.depth.ctypes.data)
    assert "sgm_mi355x:" in capfd.readouterr().err
    assert L.stub_register_count() == 0 and standin.log(L) == [] and b.untouched()


@pytest.mark.parametrize("name", sorted(SOURCE_REFUSALS))
def test_every_refusal_of_the_source_spec(host, capfd, name):
    L = host
    s, _ = make(L)
    kw = dict(SOURCE_REFUSALS[name])
    sp = source_spec(kw.pop("w", W), kw.pop("h", H), kw.pop("frames", 1), **kw)
    _refused(L, s, c_source(sp), c_target(good_target()), Buffers(good_source(), good_target()), capfd)
    L.sgm_destroy(s)


@pytest.mark.parametrize("name", sorted(TARGET_REFUSALS))
def test_every_refusal_of_the_target_spec(host, capfd, name):
    L = host
    s, _ = make(L)
    kw = dict(TARGET_REFUSALS[name])
    tg = good_target(kw.pop("w", 31), kw.pop("h", 17), **kw)
    _refused(L, s, c_source(good_source()), c_target(tg), Buffers(good_source(), good_target()), capfd)
    L.sgm_destroy(s)


def test_frames_count_against_the_targets_2_31_pixels(host, capfd):
    """65535 x 32768 target pixels fit one frame (2^31 - 32768) and not two"""
    L = host
    s = L.sgm_create(0)
    b = Buffers(good_source(frames=2), good_target())
    big = c_target(good_target(65535, 32768))
    L.stub_clear(); L.stub_register_clear()
    assert not depth_call(L, s, c_source(good_source(frames=2)), big, b)
    assert "target spec" in capfd.readouterr().err and L.stub_register_count() == 0 and standin.log(L) == []
    L.sgm_destroy(s)


def test_null_aliasing_misaligned_and_element_refusals(host, capfd):
    L = host
    s, _ = make(L)
    sp, tg = good_source(), good_target()
    cs, ct = c_source(sp), c_target(tg)
    b = Buffers(sp, tg)
    d, z, q = b.disp.ctypes.data, b.depth.ctypes.data, b.source.ctypes.data
    L.stub_clear(); L.stub_register_clear()
    capfd.readouterr()
    refusals = [
        lambda: depth_call(L, None, cs, ct, b), lambda: depth_call(L, s, None, ct, b), lambda: depth_call(L, s, cs, None, b),
        lambda: depth_call(L, s, cs, ct, b, depth=None),
        # an output that aliases the map (from its first to its last byte), or the other output
        lambda: depth_call(L, s, cs, ct, b, depth=d), lambda: depth_call(L, s, cs, ct, b, source=d),
        lambda: depth_call(L, s, cs, ct, b, depth=d + b.disp.nbytes - 4), lambda: depth_call(L, s, cs, ct, b, disp=z + 4 * (b.n - 1)),
        lambda: depth_call(L, s, cs, ct, b, source=z),
        # pointers off their element
        lambda: depth_call(L, s, cs, ct, b, disp=d + 2), lambda: depth_call(L, s, cs, ct, b, disp=d + 1),
        lambda: depth_call(L, s, cs, ct, b, conf=b.conf.ctypes.data + 1), lambda: depth_call(L, s, cs, ct, b, depth=z + 2),
        lambda: depth_call(L, s, cs, ct, b, source=q + 1),
    ]
    for k, call in enumerate(refusals):
        assert not call(), k
        assert "sgm_mi355x:" in capfd.readouterr().err, k
    values, fv, out = np.zeros((1, H, W), np.uint32), np.zeros(1, np.uint32), np.full(b.n, 0xA5A5A5A5, np.uint32)
    v, f, o = values.ctypes.data, fv.ctypes.data, out.ctypes.data
    g = lambda *a: L.sgm_register_gather(*a)
    gathers = [
        lambda: g(None, C.byref(cs), C.byref(ct), q, 4, v, f, o), lambda: g(s, None, C.byref(ct), q, 4, v, f, o),
        lambda: g(s, C.byref(cs), None, q, 4, v, f, o), lambda: g(s, C.byref(cs), C.byref(ct), None, 4, v, f, o),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 4, None, f, o), lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v, None, o),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v, f, None),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 0, v, f, o), lambda: g(s, C.byref(cs), C.byref(ct), q, 3, v, f, o),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 8, v, f, o), lambda: g(s, C.byref(cs), C.byref(ct), q, -1, v, f, o),
        lambda: g(s, C.byref(cs), C.byref(ct), q + 2, 4, v, f, o), lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v + 2, f, o),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 2, v + 1, f, o), lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v, f, o + 1),
        lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v, f, v), lambda: g(s, C.byref(cs), C.byref(ct), q, 4, v, f, q),
    ]
    for k, call in enumerate(gathers):
        assert not call(), k
        assert "sgm_mi355x:" in capfd.readouterr().err, k
    assert L.stub_register_count() == 0 and standin.log(L) == [] and b.untouched() and np.all(out == 0xA5A5A5A5)
    # allowed: a byte map at any address, z_min 0 with z_max +INF, the largest sides
    bytes_map, fb8 = np.zeros((1, H, W), np.uint8), np.zeros(1, np.uint8)
    assert depth_call(L, s, cs, ct, b)
    out8 = np.zeros(b.n + 1, np.uint8)
    assert g(s, C.byref(cs), C.byref(ct), q, 1, bytes_map.ctypes.data, fb8.ctypes.data, out8.ctypes.data + 1)
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_without, capfd):
    L = host_without
    s, _ = make(L)
    sp, tg = good_source(), good_target()
    cs, ct = c_source(sp), c_target(tg)
    b = Buffers(sp, tg)
    fv, values = np.zeros(1, np.uint16), np.zeros((1, H, W), np.uint16)
    capfd.readouterr()
    L.stub_clear()
    assert not depth_call(L, s, cs, ct, b)
    assert "not part of this build" in capfd.readouterr().err
    assert not L.sgm_register_gather(s, C.byref(cs), C.byref(ct), b.source.ctypes.data, 2, values.ctypes.data, fv.ctypes.data, b.depth.ctypes.data)
    assert "not part of this build" in capfd.readouterr().err
    assert standin.log(L) == [] and b.untouched()
    L.sgm_destroy(s)


def test_last_match_map_under_the_clouds_rules(host):
    L = host
    s, opt = make(L, batch=2)
    sp, tg = good_source(frames=2, doffs=0.75), good_target()
    b = Buffers(sp, tg)
    ct = c_target(tg)
    left = np.zeros((2, H, W), np.uint8)
    out = np.zeros((2, H, W), np.float32)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    L.stub_clear(); L.stub_register_clear()
    for other in (source_spec(W + 1, H, 2), source_spec(W, H - 1, 2), source_spec(H, W, 2), source_spec(W, H, 1), source_spec(W, H, 3)):
        assert not depth_call(L, s, c_source(other), ct, b, disp=None)
    assert L.stub_register_count() == 0 and standin.log(L) == [] and b.untouched()
    cs = c_source(sp)
    assert depth_call(L, s, cs, ct, b, disp=None) and L.stub_register_count() == 1
    inst_map = L.stub_register_ptr(0, 0)
    assert inst_map not in (None, out.ctypes.data)                # the instance's own final map
    # the stand-in's map is all 0: with doffs 0.75 every pixel is kept, and the result is the restatement's
    want_d, want_s = GR.register(np.zeros((2, H, W), np.float32), sp, tg)
    assert same_bits(b.depth[:b.n].view(np.float32).reshape(want_d.shape), want_d) and same_bits(b.source[:b.n].reshape(want_s.shape), want_s)
    # ... which is where stage 8 reads from
    L.stub_clear()
    got = np.zeros((H, W), np.float32)
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [inst_map]
    # after a match of both views the final left map lives elsewhere: the registration follows stage 8
    assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_both(s, left.ctypes.data, left.ctypes.data, out.ctypes.data, b.disp.ctypes.data)
    L.stub_clear(); L.stub_register_clear()
    assert depth_call(L, s, cs, ct, b, disp=None)
    both_map = L.stub_register_ptr(0, 0)
    assert both_map != inst_map
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [both_map]
    # row tiles are refused, an explicit map still works; an instance that is not initialised has no last match
    assert L.sgm_set_rows(s, 4, 12) and L.sgm_reset(s, W, H, C.byref(opt))
    assert not depth_call(L, s, cs, ct, b, disp=None)
    assert depth_call(L, s, cs, ct, b)
    assert L.sgm_set_rows(s, 0, 0)
    L.sgm_destroy(s)
    s = L.sgm_create(0)
    assert not depth_call(L, s, cs, ct, b, disp=None)
    L.sgm_destroy(s)


def test_plain_match_logs_what_it_logs_without_the_registration(host, host_without):
    """allocations and their sizes included: an instance that never registers is the instance it was"""
    import soc_project_stereo_matching_amd as S
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs, launches = [], []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        if hasattr(L, "stub_register_clear"):
            L.stub_register_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                                           conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        launches.append(standin.launches(L))
        L.sgm_destroy(s)
    assert launches[0] == launches[1] and logs[0] == logs[1] and len(launches[0]) > 10
    assert host.stub_register_count() == 0


def test_a_refused_launch_allocation_or_wait_fails_the_call_and_leaves_the_outputs(host):
    L = host
    s, opt = make(L)
    sp, tg = good_source(), good_target()
    cs, ct = c_source(sp), c_target(tg)
    b = Buffers(sp, tg)
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    fv, values = np.array([9], np.uint16), np.ones((1, H, W), np.uint16)
    out = np.full(b.n, 0xA5A5, np.uint16)
    gather = lambda: L.sgm_register_gather(s, C.byref(cs), C.byref(ct), b.source.ctypes.data, 2, values.ctypes.data, fv.ctypes.data, out.ctypes.data)
    # the first allocation of the keys, refused
    L.stub_fail_alloc_at(0)
    ok = depth_call(L, s, cs, ct, b)
    L.stub_fail_alloc_at(-1)
    assert not ok and b.untouched() and L.stub_register_count() == 0
    # the n-th launch, refused: the outputs are untouched and the instance goes on
    for nth in (0, 1):
        L.stub_register_clear()
        L.stub_register_fail_at(nth)
        for _ in range(nth):
            assert depth_call(L, s, cs, ct, Buffers(sp, tg))
        assert not depth_call(L, s, cs, ct, b) and b.untouched(), nth
    L.stub_register_fail_at(0)
    assert not gather() and np.all(out == 0xA5A5)
    assert depth_call(L, s, cs, ct, b) and not b.untouched()
    assert gather() and not np.any(out == 0xA5A5)
    # with the post pass on a stream of its own both calls wait for the result of a match that is still in flight
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    for name, call in (("depth", lambda: depth_call(L, s, cs, ct, b)), ("gather", gather)):
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        L.stub_clear()
        assert call(), name
        assert "wait_event" in [e.name for e in standin.log(L)], name
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        L.stub_clear()
        L.stub_fail_at(b"wait_event", 0)
        L.stub_register_clear()
        assert not call() and L.stub_register_count() == 0, name
        assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_register_host_is_asan_ubsan_clean(tmp_path):
    """tests/register_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in registration."""
    exe = standin.build(tmp_path, sanitize=True, exe="register_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "register_sanitize_driver.c"), STUB_REGISTER])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("register_sanitize_driver ok")
