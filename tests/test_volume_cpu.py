"""Depth fused into a TSDF volume (extension; the contract is in include/sgm_mi355x.h, sgm_volume_spec) without a GPU: the numpy
restatement tests/volume_ref.py against a plain-Python loop with every operation rounded to float32, the two scenes of the design
(a plane, a noisy surface seen from a moving rig), planted cases of the integer average and of the crossings, header / library /
Python agreement, the C host's logic on the stand-in device (tests/stub_device.c + tests/stub_volume.c) and a sanitizer run of a
stand-alone driver.  Tolerance 0 wherever the library or the stand-in is compared with the restatement."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import standin
import volume_ref as VR
from conftest import ROOT
from test_cloud_cpu import f32, div32

STUB_VOLUME = os.path.join(ROOT, "tests", "stub_volume.c")
_p, _i, _b, _z, _u = C.c_void_p, C.c_int, C.c_bool, C.c_size_t, C.c_uint32
INF, NAN = float("inf"), float("nan")


# ---- scenes (shared with tests/test_gpu_volume.py) -----------------------------------------------------------------------------

def camera(w, h, frames=1, **kw):
    """the source camera of the scenes: the field of view of the design's 70-pixel camera with fx = 40, fb = 40"""
    fx = 40.0 * w / 70.0
    return CR.spec(w, h, fx=fx, fy=fx, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, baseline=40.0 / fx, frames=frames, **kw)


def rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def moving_rig(frames):
    """identity, then poses rotated by 0.05 rad with small translations, in turn"""
    out = [VR.pose()]
    for k in range(1, frames):
        sign = -1.0 if k % 2 else 1.0
        out.append(VR.pose(rot(k % 2, sign * 0.05), (0.02 * sign, -0.01 * k, 0.03)))
    return np.stack(out)


def plane_scene():
    """the plane of the design: 36x33x20 voxels of 0.05, three frames of a fronto-parallel plane at Z = 1.03, identity poses"""
    v = VR.spec(36, 33, 20, 0.05, (-0.9, -0.825, 0.5), 0.2)
    s = CR.spec(70, 33, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=1.0, frames=3)
    disp = np.full((3, 33, 70), np.float32(40.0) / np.float32(1.03), np.float32)
    return v, s, np.stack([VR.pose()] * 3), disp


def noisy_maps(s, rng, non_finite=True):
    """disparities of a surface near Z = 1.03 with uniform noise of 0.3 on the depth; one NaN and a block of +INF"""
    shape = (s.frames, s.height, s.width)
    depth = (1.03 + rng.uniform(-0.15, 0.15, shape)).astype(np.float32)
    disp = (np.float32(CR.fb_of(s)) / depth).astype(np.float32)
    if non_finite:
        disp[0, s.height // 2, s.width // 3] = np.nan
        disp[-1, : s.height // 4, s.width // 2: s.width // 2 + max(1, s.width // 8)] = np.inf
    return disp


def noisy_scene():
    v = VR.spec(36, 33, 20, 0.05, (-0.9, -0.825, 0.5), 0.2, max_weight=2)
    s = CR.spec(70, 33, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=1.0, frames=3)
    return v, s, moving_rig(3), noisy_maps(s, np.random.default_rng(31))


# ---- the restatement against a plain loop --------------------------------------------------------------------------------------

def floor_div(a, b):
    return a // b                                                 # Python's // floors


def loop_integrate(vox, v, s, poses, disp, mask=None, conf=None):
    """The definition of include/sgm_mi355x.h as a loop over Python floats: sums, products and quotients of two float32 values are
    exact or correctly rounded in double, so rounding each to float32 once is the float32 operation."""
    fb = f32(float(np.float32(s.fx)) * float(np.float32(s.baseline)))
    fx, fy, cx, cy, doffs, z_min, z_max = (float(np.float32(x)) for x in (s.fx, s.fy, s.cx, s.cy, s.doffs, s.z_min, s.z_max))
    voxel, trunc = float(np.float32(v.voxel)), float(np.float32(v.trunc))
    o = [float(np.float32(x)) for x in v.origin]
    out = np.array(vox, np.uint32).reshape(v.nz, v.ny, v.nx).copy()
    updates = 0
    for k in range(v.nz):
        for j in range(v.ny):
            for i in range(v.nx):
                p = [f32(o[a] + f32(f32(float(n) + 0.5) * voxel)) for a, n in enumerate((i, j, k))]
                word = int(out[k, j, i])
                tq, w = (word & 0xFFFF) - (0x10000 if word & 0x8000 else 0), word >> 16
                for fr in range(s.frames):
                    P = [float(x) for x in np.asarray(poses, np.float32).reshape(-1, 12)[fr]]
                    Xp, Yp, Zp = (f32(f32(f32(f32(P[3 * r] * p[0]) + f32(P[3 * r + 1] * p[1])) + f32(P[3 * r + 2] * p[2])) + P[9 + r])
                                  for r in range(3))
                    if not math.isfinite(Zp) or not Zp > 0:
                        continue
                    u, vv = f32(f32(fx * div32(Xp, Zp)) + cx), f32(f32(fy * div32(Yp, Zp)) + cy)
                    if not (math.isfinite(u) and math.isfinite(vv)):
                        continue
                    uf, vf = math.floor(f32(u + 0.5)), math.floor(f32(vv + 0.5))
                    if not (0 <= uf < s.width and 0 <= vf < s.height):
                        continue
                    d = float(disp[fr, vf, uf])
                    if not math.isfinite(d) or (mask is not None and mask[fr, vf, uf] == 0) or (conf is not None and int(conf[fr, vf, uf]) < s.min_conf):
                        continue
                    den = f32(d + doffs)
                    if not (math.isfinite(den) and den > 0):
                        continue
                    Z = div32(fb, den)
                    if not (math.isfinite(Z) and z_min <= Z <= z_max):
                        continue
                    sdf = f32(Z - Zp)
                    if sdf < -trunc:
                        continue
                    q = int(np.rint(np.float32(f32(div32(min(sdf, trunc), trunc) * 32767.0))))
                    num, den_i = tq * w + q, w + 1
                    tq = floor_div(2 * num + den_i, 2 * den_i)
                    w = min(w + 1, v.max_weight)
                    updates += 1
                out[k, j, i] = (w << 16) | (tq & 0xFFFF)
    return out, updates


def loop_crossings(vox, v, min_weight):
    vox = np.asarray(vox, np.uint32).reshape(-1)
    voxel = float(np.float32(v.voxel))
    o = [float(np.float32(x)) for x in v.origin]
    tq = lambda word: (int(word) & 0xFFFF) - (0x10000 if int(word) & 0x8000 else 0)
    recs = []
    for n in range(vox.size):
        at = [n % v.nx, (n // v.nx) % v.ny, n // (v.nx * v.ny)]
        for a, (step, lim) in enumerate(((1, v.nx), (v.nx, v.ny), (v.nx * v.ny, v.nz))):
            if at[a] + 1 >= lim:
                continue
            m = n + step
            if (int(vox[n]) >> 16) >= min_weight and (int(vox[m]) >> 16) >= min_weight and (tq(vox[n]) < 0) != (tq(vox[m]) < 0):
                p = [f32(o[b] + f32(f32(float(at[b]) + 0.5) * voxel)) for b in range(3)]
                s = div32(float(tq(vox[n])), float(tq(vox[n]) - tq(vox[m])))
                p[a] = f32(p[a] + f32(s * voxel))
                recs.append((p[0], p[1], p[2], n * 4 + a))
    return np.array(recs, VR.SURFACE)


def small_scene(seed=5):
    v = VR.spec(8, 5, 3, 0.22, (-0.9, -0.55, 0.7), 0.25, max_weight=3)
    s = camera(24, 16, frames=3, doffs=0.25, z_min=0.5, z_max=20.0, min_conf=9)
    rng = np.random.default_rng(seed)
    disp = noisy_maps(s, rng)
    mask = (rng.random(disp.shape) < 0.85).astype(np.uint8)
    conf = rng.integers(0, 60, disp.shape).astype(np.uint16)
    return v, s, moving_rig(3), disp, mask, conf


@pytest.mark.parametrize("sides", [False, True])
def test_restatement_equals_the_loop(sides):
    v, s, poses, disp, mask, conf = small_scene()
    if not sides:
        mask = conf = None
    start = VR.empty(v)
    start[1, 2, 3] = VR.pack(-700, 2)                              # a volume that is not empty when the call begins
    got, n = VR.integrate(start, v, s, poses, disp, mask, conf)
    want, n_loop = loop_integrate(start, v, s, poses, disp, mask, conf)
    assert n == n_loop and 30 < n < 3 * 120
    assert np.array_equal(got, want)
    assert start[1, 2, 3] == VR.pack(-700, 2) and np.count_nonzero(start) == 1             # the input is only read
    for mw in (1, 2, 3):
        a, b = VR.crossings(got, v, mw), loop_crossings(got, v, mw)
        assert a.tobytes() == b.tobytes() and (mw > 2 or len(a) > 0), mw


# ---- the scenes of the design --------------------------------------------------------------------------------------------------

def test_plane_scene_gives_the_plane():
    v, s, poses, disp = plane_scene()
    vox, updates = VR.integrate(VR.empty(v), v, s, poses, disp)
    pts = VR.crossings(vox, v, 1)
    assert updates == 20154 and len(pts) == 612
    assert np.bincount(pts["id"] & 3, minlength=3).tolist() == [0, 0, 612]                  # all on axis 2, none on 0 or 1
    err = float(np.abs(pts["z"].astype(np.float64) - 1.03).max()) / v.voxel
    print("plane: max |z - 1.03| = %.3g voxel" % err)
    assert err <= 5e-4                                            # 4 x the quantisation's trunc / 32767 = 1.2e-4 voxel
    tq, w = VR.unpack(vox)
    assert set(np.unique(w)) == {0, 3} and np.all(np.diff(pts["id"].astype(np.int64)) > 0)
    # min_weight above the three frames' weight: no surface
    assert len(VR.crossings(vox, v, 4)) == 0


def test_noisy_scene_batch_equals_frame_by_frame():
    v, s, poses, disp = noisy_scene()
    vox, updates = VR.integrate(VR.empty(v), v, s, poses, disp)
    one = VR.empty(v)
    total = 0
    for f in range(3):
        s1 = CR.spec(s.width, s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, frames=1)
        one, n = VR.integrate(one, v, s1, poses[f:f + 1], disp[f:f + 1])
        total += n
    assert np.array_equal(one, vox) and total == updates and 15000 < updates < 3 * 36 * 33 * 20
    tq, w = VR.unpack(vox)
    assert w.max() == 2 and (w == 2).sum() > 1000 and (tq < 0).sum() > 1000                 # weights reach the cap
    per_axis = np.bincount(VR.crossings(vox, v, 1)["id"] & 3, minlength=3)
    assert np.all(per_axis > 300), per_axis                       # a noisy surface crosses on every axis
    assert len(VR.crossings(vox, v, 2)) < per_axis.sum()


# ---- planted cases -------------------------------------------------------------------------------------------------------------

def planted_scene(words, max_weight=65535):
    """len(words) voxels in a row at Z' = 1 under a plane at Z = 1 exactly: sdf = 0, q = 0, so the update is tq*w / (w + 1) rounded"""
    v = VR.spec(len(words), 1, 1, 1.0 / 64, (-len(words) / 128.0, -1.0 / 128, 1.0 - 1.0 / 128), 0.25, max_weight=max_weight)
    s = CR.spec(16, 8, fx=40.0, fy=40.0, cx=7.5, cy=3.5, baseline=1.0, frames=1)
    disp = np.full((1, 8, 16), 40.0, np.float32)
    return v, s, VR.pose()[None], disp, np.array([VR.pack(t, w) for t, w in words], np.uint32).reshape(1, 1, -1)


#            (tq, w) before          tq after: tq*w / (w + 1), halves up
PLANTED = [((-1, 1), 0),             # -0.5 -> 0
           ((-3, 1), -1),            # -1.5 -> -1
           ((3, 1), 2),              # 1.5 -> 2
           ((-2, 3), -1),            # -6 / 4 = -1.5 -> -1
           ((-5, 1), -2),            # -2.5 -> -2
           ((-4, 1), -2), ((-7, 2), -5), ((-8, 2), -5),           # -4.67 -> -5, -5.33 -> -5
           ((-32767, 65535), -32767), ((32767, 65535), 32767),    # 2*num + den is past int32 here
           ((-32768, 65534), -32767),           # -32767.49999
           ((-21846, 32767), -21845),                            # num = -21846 * 32767, den = 32768: ..5.33 -> -21845
           ((0, 0), 0), ((0, 7), 0)]


def test_planted_floor_division():
    v, s, poses, disp, start = planted_scene([p[0] for p in PLANTED])
    got, n = VR.integrate(start, v, s, poses, disp)
    assert n == len(PLANTED)
    tq, w = VR.unpack(got)
    assert tq.reshape(-1).tolist() == [p[1] for p in PLANTED]
    assert w.reshape(-1).tolist() == [min(p[0][1] + 1, 65535) for p in PLANTED]
    assert np.array_equal(loop_integrate(start, v, s, poses, disp)[0], got)
    for (t, wt), want in PLANTED:                                  # the definition, in exact arithmetic
        assert want == math.floor((t * wt) / (wt + 1) + 0.5) or wt > 30000


def planted_crossings():
    """tq = 0 on either side of a crossing, weights below and at min_weight, the last voxel of every axis"""
    v = VR.spec(4, 3, 2, 0.5, (1.0, -2.0, 0.25), 0.2)
    tq = np.array([[[0, -5, 0, 7], [3, 3, -1, -1], [-9, 0, 0, -2]], [[-1, -1, 5, 0], [0, 0, 0, 0], [9, -9, 9, -9]]])
    w = np.array([[[2, 2, 2, 2], [2, 1, 2, 2], [2, 2, 2, 2]], [[2, 2, 2, 2], [1, 2, 2, 2], [2, 2, 2, 0]]])
    return v, VR.pack(tq, w)


def test_planted_crossings_with_zero_on_either_side():
    v, vox = planted_crossings()
    for mw in (1, 2, 3):
        pts = VR.crossings(vox, v, mw)
        assert pts.tobytes() == loop_crossings(vox, v, mw).tobytes()
    pts = {int(p["id"]): p for p in VR.crossings(vox, v, 1)}
    # n = 0: tq 0 beside -5 along x -> s = 0, the point is the centre of voxel 0
    assert 0 in pts and (pts[0]["x"], pts[0]["y"], pts[0]["z"]) == (1.25, -1.75, 0.5)
    # n = 1: tq -5 beside 0 -> s = 1, the centre of voxel 2
    assert 4 in pts and pts[4]["x"] == 2.25
    # 0 beside 0 is no crossing (n = 9, 10 along x), neither is 0 beside 7
    assert 4 * 9 not in pts and 4 * 2 not in pts
    assert len(VR.crossings(vox, v, 3)) == 0 and 0 < len(VR.crossings(vox, v, 2)) < len(pts)


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


FIELDS = ["nx", "ny", "nz", "voxel", "origin", "trunc", "max_weight"]
OFFSETS = [0, 4, 8, 12, 16, 28, 32]


def c_volume(v):
    import soc_project_stereo_matching_amd as S
    return S.volume_spec(v.nx, v.ny, v.nz, v.voxel, v.origin, v.trunc, v.max_weight)


def c_source(s):
    import soc_project_stereo_matching_amd as S
    return S.SGMCloudSpec(s.width, s.height, s.frames, s.fx, s.fy, s.cx, s.cy, s.baseline, s.doffs, s.z_min, s.z_max, s.min_conf)


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in ("sgm_volume_bytes", "sgm_volume_integrate", "sgm_volume_points"):
        assert name in declared and hasattr(lib, name), name
    for name in ("sgmd_volume_integrate", "sgmd_volume_points", "sgmd_volume_scratch_bytes"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    for line in ("X' = ((R0*px + R1*py) + R2*pz) + t0", "q   = (int)rintf((fminf(sdf, trunc) / trunc) * 32767.0f)",
                 "tq = floor_div(2*num + den, 2*den)", "w   = min(w + 1, max_weight)"):
        assert line in text, line
    for out in ("ray-casting", "meshing", "confidence-weighted", "colour", "voxel hashing", "estimating the poses", "row tiles", "sgm_match_planes"):
        assert out in text.split("sgm_volume_spec;")[0].split("fused into a TSDF volume")[1], out
    assert C.sizeof(S.SGMVolumeSpec) == 36 and S.SURFACE_DTYPE.itemsize == 16 and S.SURFACE_DTYPE == VR.SURFACE
    assert [f[0] for f in S.SGMVolumeSpec._fields_] == FIELDS
    assert [getattr(S.SGMVolumeSpec, n).offset for n in FIELDS] == OFFSETS
    body = re.search(r"typedef struct \{([^}]*)\} sgm_volume_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == FIELDS
    assert re.search(r"typedef struct \{ float x, y, z; uint32_t id; \} sgm_surface_point;", text)
    for m in ("volume_integrate", "volume_points"):
        assert callable(getattr(S.SGMInstance, m, None)), m
    # sgm_volume_bytes is the host's range check: 4 bytes per voxel, 0 for a refused spec
    good = VR.spec(36, 33, 20, 0.05, (-0.9, -0.825, 0.5), 0.2)
    assert S.volume_bytes(c_volume(good)) == 4 * 36 * 33 * 20
    assert S.volume_bytes(c_volume(VR.spec(1024, 1024, 1024, 1e-3, (0, 0, 0), 1e-2, 65535))) == 1 << 32
    assert lib.sgm_volume_bytes(None) == 0
    for name, kw in VOLUME_REFUSALS.items():
        assert S.volume_bytes(c_volume(bad_volume(**kw))) == 0, name


def bad_volume(**kw):
    d = dict(nx=12, ny=6, nz=5, voxel=0.15, origin=(-0.9, -0.45, 0.7), trunc=0.3, max_weight=4)
    d.update(kw)
    return VR.spec(**d)


VOLUME_REFUSALS = {
    "nx 0": dict(nx=0), "nx -1": dict(nx=-1), "nx 1025": dict(nx=1025), "ny 0": dict(ny=0), "ny 1025": dict(ny=1025), "nz 0": dict(nz=0),
    "nz 1025": dict(nz=1025), "voxel 0": dict(voxel=0.0), "voxel < 0": dict(voxel=-0.1), "voxel NaN": dict(voxel=NAN), "voxel INF": dict(voxel=INF),
    "origin NaN": dict(origin=(0, NAN, 0)), "origin INF": dict(origin=(INF, 0, 0)), "origin -INF": dict(origin=(0, 0, -INF)),
    "trunc 0": dict(trunc=0.0), "trunc < 0": dict(trunc=-1.0), "trunc NaN": dict(trunc=NAN), "trunc INF": dict(trunc=INF),
    "max_weight 0": dict(max_weight=0), "max_weight 65536": dict(max_weight=65536),
}


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

class DeviceVolume(C.Structure):                                 # sgmd_volume of csrc/sgm_device.h
    _fields_ = [("nx", _i), ("ny", _i), ("nz", _i), ("voxel", C.c_float), ("origin", C.c_float * 3), ("trunc", C.c_float), ("max_weight", C.c_uint)]


class DeviceSrc(C.Structure):                                    # sgmd_cloud of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i), ("B", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "fb", "doffs", "z_min", "z_max")] + \
               [("min_conf", C.c_uint)]


def _sign(L):
    for name, (res, args) in {"sgm_volume_bytes": (_z, [_p]), "sgm_volume_integrate": (_b, [_p] * 8),
                              "sgm_volume_points": (_b, [_p] * 3 + [_u, _p, _z, _p]),
                              "stub_volume_clear": (None, []), "stub_volume_count": (_i, []), "stub_volume_kind": (_i, [_i]),
                              "stub_volume_ptr": (_p, [_i, _i]), "stub_volume_spec": (C.POINTER(DeviceVolume), [_i]),
                              "stub_volume_src": (C.POINTER(DeviceSrc), [_i]), "stub_volume_poses": (C.POINTER(C.c_float), [_i]),
                              "stub_volume_min_weight": (C.c_uint, [_i]), "stub_volume_capacity": (_z, [_i]),
                              "stub_volume_fail_at": (None, [_i]), "stub_fail_alloc_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("volumestub"), extra_sources=[STUB_VOLUME], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("volumestub_without"), flags=("-ffp-contract=off",)))


W, H = 48, 20
A5 = 0xA5A5A5A5


def good_source(frames=1, **kw):
    return camera(W, H, frames=frames, min_conf=7, **kw)


class Buffers:
    """a caller's "device" buffers on the stand-in: host memory; the volume empty (or, poison=True, 0xA5 like the other outputs)
    with 0xA5 words behind it, the point list and the count pre-filled with 0xA5"""
    def __init__(self, v, s, seed=3, poison=False):
        rng = np.random.default_rng(seed)
        self.disp = noisy_maps(s, rng)
        shape = self.disp.shape
        self.mask = (rng.random(shape) < 0.8).astype(np.uint8)
        self.conf = rng.integers(0, 14, shape).astype(np.uint16)
        self.n = max(1, v.nx * v.ny * v.nz)
        self.voxels = np.full(self.n + 4, A5, np.uint32)
        if not poison:
            self.voxels[:self.n] = 0
        self.points = np.full(4 * (3 * self.n + 4), A5, np.uint32)
        self.count = np.full(4, A5, np.uint32)

    def untouched(self):
        return bool(np.all(self.voxels == A5) and np.all(self.points == A5) and np.all(self.count == A5))

    def volume(self, v):
        assert np.all(self.voxels[self.n:] == A5)
        return self.voxels[:self.n].reshape(v.nz, v.ny, v.nx).copy()

    def records(self, written):
        """the first `written` records; everything behind them still 0xA5"""
        assert np.all(self.points[4 * written:] == A5) and np.all(self.count[1:] == A5)
        return self.points[:4 * written].view(VR.SURFACE)


def make(L, w=W, h=H, batch=1):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    opt = S.default_option(16)
    assert L.sgm_set_batch(s, batch) and L.sgm_reset(s, w, h, C.byref(opt))
    return s, opt


def integrate_call(L, s, cv, cs, poses, b, disp="own", mask=None, conf=None, voxels="own"):
    return L.sgm_volume_integrate(s, None if cv is None else C.byref(cv), None if cs is None else C.byref(cs),
                                  None if poses is None else poses.ctypes.data, b.disp.ctypes.data if isinstance(disp, str) else disp,
                                  mask, conf, b.voxels.ctypes.data if isinstance(voxels, str) else voxels)


def points_call(L, s, cv, b, min_weight=1, capacity=None, voxels="own", points="own", count="own"):
    return L.sgm_volume_points(s, None if cv is None else C.byref(cv), b.voxels.ctypes.data if isinstance(voxels, str) else voxels, min_weight,
                               b.points.ctypes.data if isinstance(points, str) else points, 3 * b.n if capacity is None else capacity,
                               b.count.ctypes.data if isinstance(count, str) else count)


def test_the_validated_specs_the_poses_and_the_callers_pointers_arrive(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: an explicit map needs no shape
    v, sp = bad_volume(), good_source(frames=3)
    b = Buffers(v, sp)
    cv, cs = c_volume(v), c_source(sp)
    poses = moving_rig(3)
    L.stub_clear(); L.stub_volume_clear()
    assert integrate_call(L, s, cv, cs, poses, b, mask=b.mask.ctypes.data, conf=b.conf.ctypes.data)
    assert L.stub_volume_count() == 1 and L.stub_volume_kind(0) == 0
    assert [L.stub_volume_ptr(0, k) for k in range(5)] == [b.disp.ctypes.data, b.mask.ctypes.data, b.conf.ctypes.data, b.voxels.ctypes.data,
                                                           poses.ctypes.data]
    assert np.array_equal(np.ctypeslib.as_array(L.stub_volume_poses(0), (36,)), poses.reshape(-1))             # the poses as given
    d, t = L.stub_volume_src(0).contents, L.stub_volume_spec(0).contents
    assert (d.W, d.H, d.B, d.min_conf) == (W, H, 3, 7) and np.float32(d.fb) == CR.fb_of(sp)
    assert bytes(t) == bytes(cv)
    assert standin.log(L) == []                                   # the integration allocates nothing and copies nothing
    # the stand-in computes for real: what arrived is the restatement
    want, updates = VR.integrate(VR.empty(v), v, sp, poses, b.disp, b.mask, b.conf)
    assert updates > 100 and np.array_equal(b.volume(v), want)
    # the surface list: one allocation (the tile scratch; the first allocation of a buffer drains the instance's stream)
    pts = VR.crossings(want, v, 1)
    assert len(pts) > 20
    assert points_call(L, s, cv, b, min_weight=1)
    assert L.stub_volume_count() == 2 and L.stub_volume_kind(1) == 1 and L.stub_volume_min_weight(1) == 1 and L.stub_volume_capacity(1) == 3 * b.n
    assert [L.stub_volume_ptr(1, k) for k in (0, 2, 3)] == [b.voxels.ctypes.data, b.points.ctypes.data, b.count.ctypes.data]
    scratch = L.stub_volume_ptr(1, 1)
    assert scratch not in (None, b.points.ctypes.data)
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", 0)]                                          # 8 bytes, logged in KiB
    assert b.count[0] == len(pts) and b.records(len(pts)).tobytes() == pts.tobytes()
    # the scratch is kept: the same call again, and a smaller volume, allocate nothing
    L.stub_clear()
    assert points_call(L, s, cv, b, min_weight=2) and b.count[0] == len(VR.crossings(want, v, 2))
    small = bad_volume(nx=4, ny=3, nz=2)
    assert points_call(L, s, c_volume(small), b, capacity=0, points=None)
    assert standin.launches(L, drop=()) == [] and L.stub_volume_ptr(3, 1) == scratch
    # a larger one (more than one tile of 2048 voxels) grows it: a drain and an allocation of the new size
    big = bad_volume(nx=64, ny=40, nz=50, voxel=0.03, origin=(-0.96, -0.6, 0.5))       # 128000 voxels: 63 tiles, 504 bytes
    b2 = Buffers(big, sp)
    assert integrate_call(L, s, c_volume(big), cs, poses, b2)
    L.stub_clear()
    assert points_call(L, s, c_volume(big), b2)
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", 0)] and L.stub_volume_ptr(5, 1) != scratch
    want2, _ = VR.integrate(VR.empty(big), big, sp, poses, b2.disp)
    pts2 = VR.crossings(want2, big, 1)
    assert np.array_equal(b2.volume(big), want2) and b2.count[0] == len(pts2) > 500 and b2.records(len(pts2)).tobytes() == pts2.tobytes()
    L.sgm_destroy(s)


def test_capacity_clips_the_list_and_never_the_count(host):
    L = host
    s = L.sgm_create(0)
    v, sp = bad_volume(), good_source(frames=2)
    cv = c_volume(v)
    b = Buffers(v, sp)
    assert integrate_call(L, s, cv, c_source(sp), moving_rig(2), b)
    pts = VR.crossings(b.volume(v), v, 1)
    for cap in (0, len(pts) - 1, len(pts), len(pts) + 5):
        b.points[:] = A5
        b.count[:] = A5
        assert points_call(L, s, cv, b, capacity=cap)
        written = min(cap, len(pts))
        assert b.count[0] == len(pts) and b.records(written).tobytes() == pts[:written].tobytes(), cap
    L.sgm_destroy(s)


SOURCE_REFUSALS = {
    "src width 0": dict(w=0), "src width 65536": dict(w=65536), "src height 0": dict(h=0), "src frames 0": dict(frames=0),
    "src frames 65": dict(frames=65), "src fx NaN": dict(fx=NAN), "src baseline 0": dict(baseline=0.0), "src doffs NaN": dict(doffs=NAN),
    "src z_min < 0": dict(z_min=-1.0), "src z_max == z_min": dict(z_min=5.0, z_max=5.0), "src min_conf 65536": dict(min_conf=65536),
}


def _refused(L, s, cv, cs, poses, b, capfd, points_too=True):
    """the entry points answer false with a message, queue nothing and leave the outputs alone"""
    L.stub_clear(); L.stub_volume_clear()
    capfd.readouterr()
    assert not integrate_call(L, s, cv, cs, poses, b)
    assert "sgm_mi355x:" in capfd.readouterr().err
    if points_too:
        assert not points_call(L, s, cv, b)
        assert "sgm_mi355x:" in capfd.readouterr().err
    assert L.stub_volume_count() == 0 and standin.log(L) == [] and b.untouched()


@pytest.mark.parametrize("name", sorted(VOLUME_REFUSALS))
def test_every_refusal_of_the_volume_spec(host, capfd, name):
    L = host
    s, _ = make(L)
    _refused(L, s, c_volume(bad_volume(**VOLUME_REFUSALS[name])), c_source(good_source()), moving_rig(1),
             Buffers(bad_volume(), good_source(), poison=True), capfd)
    L.sgm_destroy(s)


@pytest.mark.parametrize("name", sorted(SOURCE_REFUSALS))
def test_every_refusal_of_the_source_spec(host, capfd, name):
    L = host
    s, _ = make(L)
    kw = dict(SOURCE_REFUSALS[name])
    base = good_source()
    frames = kw.pop("frames", 1)
    sp = CR.spec(kw.pop("w", W), kw.pop("h", H), **{**dict(fx=base.fx, fy=base.fy, cx=base.cx, cy=base.cy, baseline=base.baseline), **kw},
                 frames=frames)
    _refused(L, s, c_volume(bad_volume()), c_source(sp), moving_rig(max(1, frames)), Buffers(bad_volume(), good_source(), poison=True), capfd,
             points_too=False)
    L.sgm_destroy(s)


def test_64_frames_are_taken_and_a_non_finite_pose_entry_is_not(host, capfd):
    L = host
    s = L.sgm_create(0)
    v = bad_volume()
    sp = camera(12, 8, frames=64)
    b = Buffers(v, sp)
    poses = moving_rig(64)
    assert integrate_call(L, s, c_volume(v), c_source(sp), poses, b)
    want, _ = VR.integrate(VR.empty(v), v, sp, poses, b.disp)
    assert np.array_equal(b.volume(v), want)
    L.stub_clear(); L.stub_volume_clear()
    bp = Buffers(v, sp, poison=True)
    for at in (0, 5, 11, 12 * 63 + 11, 12 * 17 + 9):
        for bad in (NAN, INF, -INF):
            p = poses.copy()
            p.reshape(-1)[at] = bad
            capfd.readouterr()
            assert not integrate_call(L, s, c_volume(v), c_source(sp), p, bp), (at, bad)
            assert "not finite" in capfd.readouterr().err
    assert L.stub_volume_count() == 0 and standin.log(L) == [] and bp.untouched()
    L.sgm_destroy(s)


def test_null_aliasing_and_misaligned_refusals(host, capfd):
    L = host
    s, _ = make(L)
    v, sp = bad_volume(), good_source()
    cv, cs = c_volume(v), c_source(sp)
    b = Buffers(v, sp, poison=True)
    poses = moving_rig(1)
    d, x, q, k = b.disp.ctypes.data, b.voxels.ctypes.data, b.points.ctypes.data, b.count.ctypes.data
    m8 = np.ones(4 * b.n + 64, np.uint8)                          # a byte map large enough to hold a volume inside it
    L.stub_clear(); L.stub_volume_clear()
    capfd.readouterr()
    ic = lambda **kw: integrate_call(L, s, cv, cs, poses, b, **kw)
    pc = lambda **kw: points_call(L, s, cv, b, **kw)
    refusals = [
        lambda: integrate_call(L, None, cv, cs, poses, b), lambda: integrate_call(L, s, None, cs, poses, b),
        lambda: integrate_call(L, s, cv, None, poses, b), lambda: integrate_call(L, s, cv, cs, None, b), lambda: ic(voxels=None),
        # a volume that aliases a map, from its first to its last byte
        lambda: ic(voxels=d), lambda: ic(voxels=d + b.disp.nbytes - 4), lambda: ic(disp=x + 4 * (b.n - 1)),
        lambda: ic(mask=x + 4 * b.n - 1), lambda: ic(conf=x), lambda: ic(voxels=m8.ctypes.data + 8, mask=m8.ctypes.data),
        # pointers off their element
        lambda: ic(disp=d + 2), lambda: ic(disp=d + 1), lambda: ic(conf=b.conf.ctypes.data + 1), lambda: ic(voxels=x + 2), lambda: ic(voxels=x + 1),
        # the surface list
        lambda: points_call(L, None, cv, b), lambda: points_call(L, s, None, b), lambda: pc(voxels=None), lambda: pc(count=None),
        lambda: pc(points=None), lambda: pc(min_weight=0), lambda: pc(min_weight=65536),
        lambda: pc(voxels=x + 2), lambda: pc(points=q + 8), lambda: pc(points=q + 4), lambda: pc(count=k + 2),
        lambda: pc(points=x), lambda: pc(count=x + 8), lambda: pc(count=q + 16), lambda: pc(points=x + (-x % 16)),
    ]
    for n, call in enumerate(refusals):
        assert not call(), n
        assert "sgm_mi355x:" in capfd.readouterr().err, n
    assert L.stub_volume_count() == 0 and standin.log(L) == [] and b.untouched()
    # allowed: byte and confidence maps at any address of their element, a list of 0 records without a buffer, the count right
    # behind the records asked for
    b = Buffers(v, sp)
    assert integrate_call(L, s, cv, cs, poses, b, mask=m8.ctypes.data + 1, conf=b.conf.ctypes.data)
    assert points_call(L, s, cv, b, points=None, capacity=0) and b.count[0] > 0
    assert points_call(L, s, cv, b, capacity=2, count=b.points.ctypes.data + 32)
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_without, capfd):
    L = host_without
    s, _ = make(L)
    v, sp = bad_volume(), good_source()
    b = Buffers(v, sp, poison=True)
    capfd.readouterr()
    L.stub_clear()
    assert not integrate_call(L, s, c_volume(v), c_source(sp), moving_rig(1), b)
    assert "not part of this build" in capfd.readouterr().err
    assert not points_call(L, s, c_volume(v), b)
    assert "not part of this build" in capfd.readouterr().err
    assert standin.log(L) == [] and b.untouched()
    assert L.sgm_volume_bytes(C.byref(c_volume(v))) == 4 * b.n      # host only: no kernels needed
    L.sgm_destroy(s)


def test_last_match_map_under_the_clouds_rules(host):
    """d_disp == NULL after every kind of match"""
    L = host
    s, opt = make(L, batch=2)
    v = VR.spec(12, 6, 8, 0.15, (-0.9, -0.45, 52.9), 0.3)         # the stand-in's map is all 0: with doffs 0.75 every Z is 40 / 0.75
    sp = good_source(frames=2, doffs=0.75)
    cv, cs = c_volume(v), c_source(sp)
    b = Buffers(v, sp)
    poses = moving_rig(2)
    left = np.zeros((2, H, W), np.uint8)
    out, conf = np.zeros((2, H, W), np.float32), np.zeros((2, H, W), np.uint16)
    want, updates = VR.integrate(VR.empty(v), v, sp, poses, np.zeros((2, H, W), np.float32))
    assert updates > 200 and len(VR.crossings(want, v, 1)) > 10
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    L.stub_clear(); L.stub_volume_clear()
    for other in (camera(W + 1, H, 2), camera(W, H - 1, 2), camera(H, W, 2), camera(W, H, 1), camera(W, H, 3)):
        assert not integrate_call(L, s, cv, c_source(other), moving_rig(3), b, disp=None)
    assert L.stub_volume_count() == 0 and standin.log(L) == [] and np.all(b.voxels[:b.n] == 0)
    assert integrate_call(L, s, cv, cs, poses, b, disp=None) and L.stub_volume_count() == 1
    inst_map = L.stub_volume_ptr(0, 0)
    assert inst_map not in (None, out.ctypes.data)                # the instance's own final map
    assert np.array_equal(b.volume(v), want)
    # ... which is where stage 8 reads from
    L.stub_clear()
    got = np.zeros((H, W), np.float32)
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [inst_map]
    # the other matches that leave their result in the instance: asynchronous, with a confidence
    for k, call in enumerate((lambda: L.sgm_match_async(s, left.ctypes.data, left.ctypes.data, out.ctypes.data) and L.sgm_match_wait(s),
                              lambda: L.sgm_match_confidence(s, left.ctypes.data, left.ctypes.data, out.ctypes.data, conf.ctypes.data))):
        assert L.sgm_reset(s, W, H, C.byref(opt)) and call(), k
        L.stub_volume_clear()
        b.voxels[:b.n] = 0
        assert integrate_call(L, s, cv, cs, poses, b, disp=None) and L.stub_volume_ptr(0, 0) is not None, k
        assert np.array_equal(b.volume(v), want), k
    # after a match of both views the final left map lives elsewhere: the integration follows stage 8
    assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_both(s, left.ctypes.data, left.ctypes.data, out.ctypes.data, b.disp.ctypes.data)
    L.stub_clear(); L.stub_volume_clear()
    assert integrate_call(L, s, cv, cs, poses, b, disp=None)
    both_map = L.stub_volume_ptr(0, 0)
    assert both_map != inst_map
    assert L.sgm_read_stage(s, 8, got.ctypes.data, got.nbytes) == got.nbytes
    assert [e.b for e in standin.log(L) if e.name == "d2h"] == [both_map]
    # row tiles are refused, an explicit map still works; an instance that is not initialised has no last match
    assert L.sgm_set_rows(s, 4, 12) and L.sgm_reset(s, W, H, C.byref(opt))
    assert not integrate_call(L, s, cv, cs, poses, b, disp=None)
    assert integrate_call(L, s, cv, cs, poses, b)
    assert L.sgm_set_rows(s, 0, 0)
    L.sgm_destroy(s)
    s = L.sgm_create(0)
    assert not integrate_call(L, s, cv, cs, poses, b, disp=None)
    L.sgm_destroy(s)


def test_plain_match_logs_what_it_logs_without_the_volume(host, host_without):
    """allocations and their sizes included: an instance that never fuses is the instance it was"""
    import soc_project_stereo_matching_amd as S
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs, launches = [], []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        if hasattr(L, "stub_volume_clear"):
            L.stub_volume_clear()
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
    assert host.stub_volume_count() == 0


def test_a_refused_launch_allocation_or_wait_fails_the_call_and_leaves_the_outputs(host):
    L = host
    s, opt = make(L)
    v, sp = bad_volume(), good_source()
    cv, cs = c_volume(v), c_source(sp)
    poses = moving_rig(1)
    full = Buffers(v, sp)
    assert integrate_call(L, s, cv, cs, poses, full)              # a volume with a surface, for the list
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_match(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    b = Buffers(v, sp, poison=True)
    points = lambda: points_call(L, s, cv, b, voxels=full.voxels.ctypes.data)
    # the first allocation of the scratch, refused
    L.stub_volume_clear()
    L.stub_fail_alloc_at(0)
    ok = points()
    L.stub_fail_alloc_at(-1)
    assert not ok and b.untouched() and L.stub_volume_count() == 0
    # a launch, refused: the outputs are untouched and the instance goes on
    L.stub_volume_fail_at(0)
    assert not integrate_call(L, s, cv, cs, poses, b) and b.untouched()
    L.stub_volume_fail_at(0)
    assert not points() and b.untouched()
    assert points() and b.count[0] == len(VR.crossings(full.volume(v), v, 1)) > 0
    # with the post pass on a stream of its own both calls wait for the result of a match that is still in flight
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    for name, call in (("integrate", lambda: integrate_call(L, s, cv, cs, poses, full)), ("points", points)):
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        L.stub_clear()
        assert call(), name
        assert "wait_event" in [e.name for e in standin.log(L)], name
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        L.stub_clear()
        L.stub_fail_at(b"wait_event", 0)
        L.stub_volume_clear()
        assert not call() and L.stub_volume_count() == 0, name
        assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


def test_the_stand_in_agrees_on_the_planted_cases(host):
    L = host
    s = L.sgm_create(0)
    v, sp, poses, disp, start = planted_scene([p[0] for p in PLANTED])
    vox = start.reshape(-1).copy()
    assert L.sgm_volume_integrate(s, C.byref(c_volume(v)), C.byref(c_source(sp)), poses.ctypes.data, disp.ctypes.data, None, None, vox.ctypes.data)
    assert np.array_equal(vox, VR.integrate(start, v, sp, poses, disp)[0].reshape(-1))
    v, vox = planted_crossings()
    b = Buffers(v, sp)
    b.voxels[:b.n] = vox.reshape(-1)
    for mw in (1, 2, 3):
        want = VR.crossings(vox, v, mw)
        b.points[:] = A5
        assert points_call(L, s, c_volume(v), b, min_weight=mw) and b.count[0] == len(want)
        assert b.records(len(want)).tobytes() == want.tobytes()
    L.sgm_destroy(s)


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_volume_host_is_asan_ubsan_clean(tmp_path):
    """tests/volume_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in volume."""
    exe = standin.build(tmp_path, sanitize=True, exe="volume_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "volume_sanitize_driver.c"), STUB_VOLUME])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("volume_sanitize_driver ok")
