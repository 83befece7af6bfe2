"""A window of the TSDF volume (extension; the contract is the window section of include/sgm_mi355x.h) without a GPU: the numpy
restatement tests/window_ref.py against plain Python loops, header / library / Python agreement, the C host's logic and the driver
on the stand-in device (tests/stub_device.c + stub_window.c), a sanitizer run of a stand-alone driver, the kernel's compile-time
resources, and -- on the restatements alone -- the three properties the device tests rest on, with the conditions that make them
about something: windowing commutes with integration on a dyadic lattice, what leaves plus what stays is the whole mesh, and a
rig that walks out of its first box.  Tolerance 0: words and bytes are compared."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import color_ref as KR
import mesh_ref as MR
import standin
import volume_ref as VR
import window_ref as WR
from conftest import ROOT
from test_color_cpu import STUB_COLOR, STUB_MESH, Held, images_of, planted_start
from test_raycast_cpu import STUB_RAYCAST
from test_volume_cpu import STUB_VOLUME, DeviceVolume, VOLUME_REFUSALS, bad_volume, c_volume, camera, moving_rig, noisy_maps

STUB_WINDOW = os.path.join(ROOT, "tests", "stub_window.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
NAN = float("nan")


# ---- scenes (shared with tests/test_gpu_volume_window.py) ----------------------------------------------------------------------

COMMUTE_OFFSETS = ((4, -3, 2), (-5, 0, 0), (1, 1, 1), (0, 8, -4))
TILING_SHIFTS = ((7, 0, 0), (7, -6, 5), (-8, 6, -5), (0, -7, 4))


@functools.lru_cache(maxsize=None)
def dyadic_scene():
    """(v, s, poses, disp, voxels): the 36 x 33 x 20 volume on a lattice of 1/16 whose origin is a multiple of it, three noisy
    frames of the moving rig, a planted start"""
    v = VR.spec(36, 33, 20, 0.0625, (-1.125, -1.0, 0.5), 0.25, max_weight=4)
    s = camera(70, 33, frames=3)
    rng = np.random.default_rng(404)
    disp = noisy_maps(s, rng)
    vox0 = planted_start(v, rng)[0]
    vox0.setflags(write=False)
    return v, s, moving_rig(3), disp, vox0


def inside_of(src, offset, dims):
    """bool [dims]: the window's voxels that lie inside the source"""
    return WR.window(np.ones((src.nz, src.ny, src.nx), np.uint32), src, offset, dims) != 0


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """(v, words): the sphere of the mesh's tests in 20 x 17 x 12 voxels, 3 % of them emptied, on a dyadic lattice"""
    _, words = MR.sphere((20, 17, 12))
    rng = np.random.default_rng(505)
    words = np.where(rng.random(words.shape) < 0.03, 0, words).astype(np.uint32)
    words.setflags(write=False)
    return VR.spec(20, 17, 12, 0.0625, (-1.125, 0.5, 2.0), 0.25), words


def parts_of(v, shift):
    """the boxes that leave, then the box that stays"""
    stay = WR.stay_box(v, shift)
    return WR.leaving(v, shift) + ([stay] if stay else [])


def triangle_floats(vert, tri):
    """the triangles as rows of nine floats (three positions), sorted"""
    p = np.stack([vert["x"], vert["y"], vert["z"]], axis=1).astype(np.float32)
    rows = p[tri["v"].astype(np.int64)].reshape(-1, 9)
    return np.ascontiguousarray(rows[np.lexsort(rows.T[::-1])]) if len(rows) else rows


WALK_FRAMES, WALK_STEP, WALK_FOCUS, WALK_GRANULE, WALK_MARGIN = 7, (0.21, 0.06), 1.125, 4, 2


@functools.lru_cache(maxsize=None)
def walk_scene():
    """(v, s1, poses, disp, image): a rig that translates along x, with some y, past a wall wider than the volume: every frame
    sees a noisy surface near Z = 1.03 in front of wherever it stands.  s1 is the camera of one frame."""
    v = VR.spec(36, 33, 20, 0.0625, (-1.125, -1.0, 0.5), 0.25, max_weight=4)
    s = camera(70, 33, frames=WALK_FRAMES)
    rng = np.random.default_rng(606)
    disp, image = noisy_maps(s, rng), images_of(s, rng, 4)
    poses = np.stack([VR.pose(np.eye(3), (-WALK_STEP[0] * f, -WALK_STEP[1] * f, 0.0)) for f in range(WALK_FRAMES)])
    return v, camera(70, 33, frames=1), poses, disp, image


def walk(window, integrate, mesh):
    """The documented loop, once per frame: follow; window and mesh each box that leaves; shift; integrate the frame.
    window(spec, offset, dims, vox, col) -> (spec, vox, col);  integrate(spec, f, vox, col) -> (vox, col);
    mesh(spec, vox, col) -> (vertices, triangles, rgba).  Returns per step (shift, spec, vox, col, [(lo, n, vertices, triangles, rgba)])."""
    spec, _, poses, _, _ = walk_scene()
    vox = col = np.zeros((spec.nz, spec.ny, spec.nx), np.uint32)
    steps = []
    for f in range(WALK_FRAMES):
        shift = WR.follow(spec, poses[f], WALK_FOCUS, WALK_GRANULE, WALK_MARGIN)
        streamed = []
        for lo, n in WR.leaving(spec, shift):
            part = window(spec, lo, n, vox, col)
            streamed.append((lo, n) + tuple(mesh(*part)))
        if any(shift):
            spec, vox, col = window(spec, shift, (spec.nx, spec.ny, spec.nz), vox, col)
        vox, col = integrate(spec, f, vox, col)
        steps.append((shift, spec, vox, col, streamed))
    return steps


def ref_window(spec, offset, dims, vox, col):
    return WR.window_spec(spec, offset, dims), WR.window(vox, spec, offset, dims), WR.window(col, spec, offset, dims)


def ref_integrate(spec, f, vox, col):
    _, s1, poses, disp, image = walk_scene()
    return KR.integrate(vox, col, spec, s1, poses[f:f + 1], disp[f:f + 1], None, None, image[f:f + 1], 4)[:2]


def ref_mesh(spec, vox, col):
    vert, tri = MR.mesh(vox, spec, 1)
    return vert, tri, KR.colors(vox, col, spec, vert["id"], 8)


@functools.lru_cache(maxsize=None)
def walk_reference():
    return walk(ref_window, ref_integrate, ref_mesh)


# ---- the restatement against plain loops ---------------------------------------------------------------------------------------

def loop_window(words, src, offset, dims):
    words = np.asarray(words, np.uint32).reshape(src.nz, src.ny, src.nx)
    out = np.full((dims[2], dims[1], dims[0]), 0xDEADBEEF, np.uint32)
    for k in range(dims[2]):
        for j in range(dims[1]):
            for i in range(dims[0]):
                si, sj, sk = i + offset[0], j + offset[1], k + offset[2]
                out[k, j, i] = words[sk, sj, si] if 0 <= si < src.nx and 0 <= sj < src.ny and 0 <= sk < src.nz else 0
    return out


def test_restatement_equals_the_loops():
    rng = np.random.default_rng(7)
    shapes = [(5, 3, 2), (8, 4, 3), (13, 5, 3), (1, 1, 1)]
    for a in shapes:
        src = VR.spec(*a, 0.0625, (-1.125, -1.0, 0.5), 0.25)
        words = rng.integers(1, 1 << 32, (a[2], a[1], a[0]), dtype=np.uint64).astype(np.uint32)
        for b in shapes:
            for ox in range(-a[0] - 1, b[0] + 2):
                for oy, oz in ((0, 0), (-1, 1), (2, -1), (-a[1], 0), (0, a[2]), (b[1], 0)):
                    assert np.array_equal(WR.window(words, src, (ox, oy, oz), b), loop_window(words, src, (ox, oy, oz), b)), (a, b, ox, oy, oz)
    # the spec: the product, then the sum, in float32
    src = VR.spec(9, 8, 7, 0.05, (-0.9, 0.825, 0.5), 0.2, max_weight=11)
    w = WR.window_spec(src, (3, -7, 1 << 20), (4, 5, 6))
    assert (w.nx, w.ny, w.nz, w.voxel, w.trunc, w.max_weight) == (4, 5, 6, 0.05, 0.2, 11)
    f = np.float32
    assert [f(o) for o in w.origin] == [f(f(-0.9) + f(f(3) * f(0.05))), f(f(0.825) + f(f(-7) * f(0.05))), f(f(0.5) + f(f(1 << 20) * f(0.05)))]
    assert WR.window_spec(src, (0, 0, (1 << 20) + 1), (4, 5, 6)) is None and WR.window_spec(src, (0, 0, 0), (4, 0, 6)) is None
    assert WR.window_spec(src, (0, 0, 0), (1024, 1024, 1024)) is not None and WR.window_spec(src, (0, 0, 0), (1025, 1, 1)) is None
    # follow, against the formula spelt out in Python floats, and its refusals
    v = dyadic_scene()[0]
    for k in range(40):
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        pose = VR.pose(R, rng.uniform(-3, 3, 3))
        fz, granule, margin = float(np.float32(rng.uniform(0, 2))), int(rng.integers(1, 9)), int(rng.integers(0, 4))
        p = [float(x) for x in pose]
        want = []
        for a, n in enumerate((v.nx, v.ny, v.nz)):
            P = (p[a] * (0.0 - p[9]) + p[3 + a] * (0.0 - p[10])) + p[6 + a] * (fz - p[11])
            g = (P - v.origin[a]) / v.voxel - n / 2
            want.append(0 if abs(g) <= margin else granule * math.floor(g / granule + 0.5))
        assert WR.follow(v, pose, fz, granule, margin) == tuple(want), k
    assert WR.follow(v, VR.pose(), 1.125, 4, 2) == (0, 0, 0) and WR.follow(v, VR.pose(np.eye(3), (-0.2, 0, 0)), 1.125, 4, 2) == (4, 0, 0)
    assert WR.follow(v, VR.pose(np.eye(3), (0.126, 0, 0)), 1.125, 4, 2) == (-4, 0, 0) and WR.follow(v, VR.pose(np.eye(3), (0.125, 0, 0)), 1.125, 4, 2) == (0, 0, 0)
    for bad in (dict(pose=VR.pose(np.eye(3), (NAN, 0, 0))), dict(focus_z=float("inf")), dict(granule=0), dict(margin=-1), dict(focus_z=1e6)):
        kw = dict(pose=VR.pose(), focus_z=0.0, granule=4, margin=0)
        kw.update(bad)
        assert WR.follow(v, **kw) is None, bad


def test_leaving_and_staying_cover_every_cell_exactly_once():
    rng = np.random.default_rng(9)
    for dims in ((20, 17, 12), (5, 3, 2), (2, 2, 2), (7, 1, 4), (1, 1, 1)):
        v = VR.spec(*dims, 0.0625, (0, 0, 0), 0.25)
        cells = tuple(n - 1 for n in dims)
        shifts = [(0, 0, 0), (7, -6, 5), (-8, 6, -5), (100, 0, 0), (0, -100, 1), (1, 1, 1), (-1, -1, -1)] + [tuple(int(x) for x in rng.integers(-9, 10, 3)) for _ in range(30)]
        for shift in shifts:
            count = np.zeros(cells[::-1], np.int64)
            boxes = WR.leaving(v, shift)
            assert len(boxes) <= 3
            for lo, n in parts_of(v, shift):
                assert all(m >= 2 for m in n) and all(0 <= l and l + m <= d for l, m, d in zip(lo, n, dims))
                count[lo[2]:lo[2] + n[2] - 1, lo[1]:lo[1] + n[1] - 1, lo[0]:lo[0] + n[0] - 1] += 1
            assert np.all(count == 1), (dims, shift)
            # the cells that stay are the cells of the shifted volume that were inside the old one
            stay = WR.stay_box(v, shift)
            if stay:
                inside = inside_of(v, shift, dims)
                lo, n = stay
                assert np.all(inside[lo[2] - shift[2]:lo[2] - shift[2] + n[2], lo[1] - shift[1]:lo[1] - shift[1] + n[1],
                                     lo[0] - shift[0]:lo[0] - shift[0] + n[0]])
                assert inside.sum() == n[0] * n[1] * n[2] or any(d == 1 for d in dims)
    v = sphere_scene()[0]
    assert WR.leaving(v, (7, -6, 5)) == [((0, 0, 0), (8, 17, 12)), ((7, 10, 0), (13, 7, 12)), ((7, 0, 0), (13, 11, 6))]
    assert WR.stay_box(v, (7, -6, 5)) == ((7, 0, 5), (13, 11, 7)) and WR.leaving(v, (0, 0, 0)) == []


# ---- the three properties, on the restatements ---------------------------------------------------------------------------------

def test_windowing_commutes_with_integration_on_a_dyadic_lattice(capsys):
    v, s, poses, disp, vox0 = dyadic_scene()
    dims = (v.nx, v.ny, v.nz)
    fused = VR.integrate(vox0, v, s, poses, disp)[0]
    assert (fused != vox0).sum() > 3000
    for offset in COMMUTE_OFFSETS:
        w = WR.window_spec(v, offset, dims)
        first = WR.window(fused, v, offset, dims)
        second = VR.integrate(WR.window(vox0, v, offset, dims), w, s, poses, disp)[0]
        inside = inside_of(v, offset, dims)
        assert np.array_equal(first[inside], second[inside]), offset
        assert np.all(first[~inside] == 0) and (second[~inside] != 0).sum() >= 10, (offset, (second[~inside] != 0).sum())
        for mine, theirs, o, n in zip(VR.centres(w), VR.centres(v), offset, dims):   # the same floats where both exist
            lo, hi = max(0, -o), min(n, n - o)
            assert hi > lo and mine[lo:hi].tobytes() == theirs[lo + o:hi + o].tobytes(), offset
    # an observation, not a contract: on the lattice of 0.05 the centres agree to rounding only, and isolated words differ
    v5 = VR.spec(36, 33, 20, 0.05, (-0.9, -0.825, 0.5), 0.2, max_weight=4)
    fused5 = VR.integrate(vox0, v5, s, poses, disp)[0]
    differ = 0
    for offset in COMMUTE_OFFSETS:
        second = VR.integrate(WR.window(vox0, v5, offset, dims), WR.window_spec(v5, offset, dims), s, poses, disp)[0]
        inside = inside_of(v5, offset, dims)
        differ += int((WR.window(fused5, v5, offset, dims)[inside] != second[inside]).sum())
    with capsys.disabled():
        print(f"\n[window] voxel 0.05, four offsets: {differ} words inside differ between window-then-integrate and integrate-then-window")


def test_what_leaves_plus_what_stays_is_the_whole_mesh():
    v, words = sphere_scene()
    whole = triangle_floats(*MR.mesh(words, v, 1))
    assert len(whole) > 1000
    for shift in TILING_SHIFTS:
        rows = []
        for lo, n in parts_of(v, shift):
            part = triangle_floats(*MR.mesh(WR.window(words, v, lo, n), WR.window_spec(v, lo, n), 1))
            assert len(part) >= 100, (shift, lo, n, len(part))
            rows.append(part)
        rows = np.concatenate(rows)
        assert rows[np.lexsort(rows.T[::-1])].tobytes() == whole.tobytes(), shift


def test_the_walk_leaves_its_first_box_and_streams_a_surface():
    steps = walk_reference()
    v = walk_scene()[0]
    shifts = [s[0] for s in steps]
    assert sum(any(sh) for sh in shifts) >= 2 and any(sh[1] for sh in shifts), shifts
    assert max((len(tri) for s in steps for _, _, _, tri, _ in s[4]), default=0) >= 50
    assert -walk_scene()[2][-1][9] > v.origin[0] + v.nx * v.voxel  # the rig ends up outside the box it started in
    assert sum(sh[0] for sh in shifts) >= v.nx // 2
    last = steps[-1]
    assert last[1].origin[0] == v.origin[0] + sum(sh[0] for sh in shifts) * v.voxel
    assert (VR.unpack(last[2])[1] > 0).sum() > 2000 and (KR.unpack(last[3])[3] > 0).sum() > 1000
    assert any((rgba >> 24 == 0xFF).sum() > 20 for s in steps for *_, rgba in s[4])


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


ENTRIES = ("sgm_volume_window", "sgm_volume_window_spec", "sgm_volume_follow", "sgm_volume_leaving")


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name), name
    assert hasattr(lib, "sgmd_volume_window") and callable(getattr(S.SGMInstance, "volume_window", None))
    for name in ("volume_window_spec", "volume_follow", "volume_leaving", "SGMVolumeBox"):
        assert name in S.__all__ and hasattr(S, name), name
    assert C.sizeof(S.SGMVolumeBox) == 24 and [f[0] for f in S.SGMVolumeBox._fields_] == ["lo", "n"] and S.SGMVolumeBox.n.offset == 12
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    assert re.search(r"typedef struct \{ int32_t lo\[3\]; int32_t n\[3\]; \} sgm_volume_box;", text)
    head = "a window of the TSDF volume: a volume that follows the rig and streams out what leaves"
    assert text.count(head) == 1 and text.index(head) > text.index("bool sgm_volume_colors(")
    block = text.split(head)[1].split("typedef struct { int32_t lo[3]")[0]
    for line in ("origin_a = src.origin_a + (float)offset_a * src.voxel", "P_i     = (R[0][i]*(0 - t0) + R[1][i]*(0 - t1)) + R[2][i]*(focus_z - t2)",
                 "g_a     = (P_a - origin_a) / voxel - n_a / 2", "shift_a = 0 if |g_a| <= margin, else granule * floor(g_a / granule + 0.5)",
                 "s > 0:  the cells [0, min(s, c)) leave and [min(s, c), c) stay", "s < 0:  the cells [max(c + s, 0), c) leave and [0, max(c + s, 0)) stay",
                 "every destination word is written exactly once", "power of two", "multiple of 4", "|offset_a| > 2^20", "Not part of it:",
                 "1. sgm_volume_follow", "2. for each box of sgm_volume_leaving", "3. sgm_volume_mesh / sgm_volume_colors", "4. sgm_volume_window"):
        assert line in block, line
    # the volume's own section no longer lists a moving volume as missing: it points here
    volume = text.split("sgm_volume_spec;")[0].split("fused into a TSDF volume")[1]
    assert "a moving volume" not in volume and "sgm_volume_window below" in volume
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_host.c")) as fh:
        assert "#pragma weak sgmd_volume_window\n" in fh.read()
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "Makefile")) as fh:
        assert re.search(r"^HIP_UNITS := .*\bsgm_window\b", fh.read(), re.M)
    # the host-only calls through the package, against the restatement
    v = dyadic_scene()[0]
    for offset, dims in (((4, -3, 2), (36, 33, 20)), ((-5, 0, 0), (7, 9, 1024)), ((1 << 20, -(1 << 20), 1), (1, 1, 1))):
        got, want = S.volume_window_spec(c_volume(v), offset, dims), WR.window_spec(v, offset, dims)
        assert bytes(got) == bytes(c_volume(want)), (offset, dims)
    assert S.volume_window_spec(c_volume(v), (0, 0, (1 << 20) + 1), (4, 4, 4)) is None
    rng = np.random.default_rng(3)
    for k in range(60):
        pose = VR.pose(np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.uniform(-3, 3, 3))
        fz, granule, margin = float(rng.uniform(0, 2)), int(rng.integers(1, 9)), int(rng.integers(0, 4))
        assert S.volume_follow(c_volume(v), pose, fz, granule, margin) == WR.follow(v, pose, fz, granule, margin), k
        shift = tuple(int(x) for x in rng.integers(-40, 41, 3))
        assert S.volume_leaving(c_volume(v), shift) == WR.leaving(v, shift), shift
    assert S.volume_follow(c_volume(v), VR.pose(), 0.0, 0, 0) is None and S.volume_leaving(c_volume(bad_volume(nx=0)), (1, 0, 0)) is None


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

def _sign(L):
    for name, (res, args) in {"sgm_volume_window": (_b, [_p] * 9), "sgm_volume_window_spec": (_b, [_p] * 4), "sgm_volume_bytes": (_z, [_p]),
                              "stub_window_clear": (None, []), "stub_window_count": (_i, []), "stub_window_ptr": (_p, [_i, _i]),
                              "stub_window_int": (_i, [_i, _i]), "stub_window_volume": (C.POINTER(DeviceVolume), [_i]),
                              "stub_window_fail_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("windowstub"), extra_sources=[STUB_WINDOW], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("windowstub_without"), flags=("-ffp-contract=off",)))


def int3(t):
    return None if t is None else (C.c_int32 * 3)(*t)


class Call:
    """the arrays of one window of the dyadic scene, and the call with any argument replaced"""
    def __init__(self, L, s, offset=(4, -3, 2), dims=(36, 33, 20)):
        import soc_project_stereo_matching_amd as S
        self.L, self.s = L, s
        self.v, _, _, _, vox0 = dyadic_scene()
        rng = np.random.default_rng(1)
        self.vox0, self.col0 = vox0, rng.integers(0, 1 << 32, vox0.shape, dtype=np.uint64).astype(np.uint32)
        self.offset, self.dims = offset, dims
        self.n, self.nd = vox0.size, dims[0] * dims[1] * dims[2]
        self.src, self.src_col, self.dst, self.dst_col = Held(self.n, self.vox0), Held(self.n, self.col0), Held(self.nd), Held(self.nd)
        self.out = S.SGMVolumeSpec()
        self.all = (self.src, self.src_col, self.dst, self.dst_col)

    def untouched(self):
        return all(h.untouched() for h in self.all) and bytes(self.out) == bytes(36)

    def __call__(self, **kw):
        a = dict(s=self.s, spec=c_volume(self.v), offset=self.offset, dims=self.dims, src=self.src.ptr, src_col=self.src_col.ptr, dst=self.dst.ptr,
                 dst_col=self.dst_col.ptr, out=self.out)
        a.update(kw)
        ref = lambda t: None if t is None else C.byref(t)
        return self.L.sgm_volume_window(a["s"], ref(a["spec"]), int3(a["offset"]), int3(a["dims"]), a["src"], a["src_col"], a["dst"], a["dst_col"],
                                        ref(a["out"]))


def clear(L):
    L.stub_clear(); L.stub_window_clear()


def test_the_validated_spec_and_the_callers_pointers_arrive_and_the_stand_in_equals_the_restatement(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: a window needs no shape
    for offset, dims, color in (((4, -3, 2), (36, 33, 20), True), ((-5, 0, 0), (36, 33, 20), False), ((30, 30, 18), (13, 5, 3), True),
                                ((-2, -2, -2), (40, 37, 24), True), ((0, 0, 0), (36, 33, 20), True), ((36, 0, 0), (4, 4, 4), False)):
        c = Call(L, s, offset, dims)
        clear(L)
        assert c() if color else c(src_col=None, dst_col=None)
        assert L.stub_window_count() == 1 and standin.log(L) == []    # no scratch, no copy, no wait without a match in flight
        assert [L.stub_window_ptr(0, k) for k in range(4)] == [c.src.ptr, c.src_col.ptr if color else None, c.dst.ptr, c.dst_col.ptr if color else None]
        assert [L.stub_window_int(0, k) for k in range(6)] == list(offset) + list(dims)
        assert bytes(L.stub_window_volume(0).contents) == bytes(c_volume(c.v))
        assert bytes(c.out) == bytes(c_volume(WR.window_spec(c.v, offset, dims)))
        assert np.array_equal(c.dst.words(), WR.window(c.vox0, c.v, offset, dims).reshape(-1))
        if color:
            assert np.array_equal(c.dst_col.words(), WR.window(c.col0, c.v, offset, dims).reshape(-1))
        else:
            assert c.dst_col.untouched()
        assert c.src.untouched() and c.src_col.untouched()
        want = c_volume(c.v)                                      # dst_out may be NULL, and may be the source spec itself
        clear(L)
        assert c(out=None) and c(spec=want, out=want) and bytes(want) == bytes(c.out) and L.stub_window_count() == 2
    L.sgm_destroy(s)


def refused(c, capfd, **kw):
    """false, one line on stderr that names the entry point, nothing logged, nothing touched"""
    clear(c.L)
    capfd.readouterr()
    assert not c(**kw), kw
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("sgm_mi355x: sgm_volume_window: "), (kw, err)
    assert c.L.stub_window_count() == 0 and standin.log(c.L) == []
    assert c.untouched(), kw
    return err


def test_every_refusal_queues_nothing_and_prints_its_line(host, capfd):
    L = host
    s = L.sgm_create(0)
    c = Call(L, s)
    f = lambda **kw: refused(c, capfd, **kw)
    for kw in (dict(s=None), dict(spec=None), dict(offset=None), dict(dims=None), dict(src=None), dict(dst=None)):
        assert "NULL argument" in f(**kw)
    assert "one colour array without the other" in f(src_col=None) and "one colour array without the other" in f(dst_col=None)
    for name, bad in sorted(VOLUME_REFUSALS.items()):
        assert "the source spec is outside" in f(spec=c_volume(bad_volume(**bad))), name
    for dims in ((0, 33, 20), (36, -1, 20), (36, 33, 1025), (1025, 1, 1), (1024, 1024, 1024 + 1), (1024, 1024, 0)):
        assert "dims outside" in f(dims=dims), dims
    for offset in (((1 << 20) + 1, 0, 0), (0, -(1 << 20) - 1, 0), (0, 0, 1 << 30), (-(1 << 31), 0, 0)):
        assert "beyond 2^20" in f(offset=offset), offset
    far = VR.spec(36, 33, 20, 1e33, (3e38, 0.0, 0.0), 1.0)
    assert "origin is not finite" in f(spec=c_volume(far), offset=(1 << 20, 0, 0))
    x, k, d, e = c.src.ptr, c.src_col.ptr, c.dst.ptr, c.dst_col.ptr
    for kw in (dict(src=x + 2), dict(src_col=k + 1), dict(dst=d + 2), dict(dst_col=e + 3), dict(dst=d + 1)):
        assert "not aligned" in f(**kw), kw
    nb, db = 4 * c.n, 4 * c.nd
    for kw in (dict(dst=x), dict(dst=x + nb - 4), dict(dst=x - db + 4), dict(dst=k), dict(dst=k + nb - 4), dict(dst_col=x), dict(dst_col=x - db + 4),
               dict(dst_col=k + 16), dict(dst_col=d), dict(dst_col=d + db - 4), dict(dst=e - db + 4), dict(src=d + 64), dict(src_col=e)):
        assert "overlaps" in f(**kw), kw
    # allowed: arrays that touch their neighbours, the two source arrays one and the same, the largest offsets and dims (the
    # stand-in only logs those)
    clear(L)
    one = np.full(c.nd + c.n + c.nd, 0xA5A5A5A5, np.uint32)       # the colours' window | the source | the voxels' window
    one[c.nd:c.nd + c.n] = c.vox0.reshape(-1)
    at = one.ctypes.data + 4 * c.nd
    assert c(src=at, src_col=at, dst=at + nb, dst_col=at - db) and L.stub_window_count() == 1
    want = WR.window(c.vox0, c.v, c.offset, c.dims).reshape(-1)
    assert np.array_equal(one[:c.nd], want) and np.array_equal(one[c.nd + c.n:], want) and np.array_equal(one[c.nd:c.nd + c.n], c.vox0.reshape(-1))
    big = dict(src=1 << 44, src_col=None, dst=1 << 45, dst_col=None)
    assert c(spec=c_volume(VR.spec(1024, 1024, 1024, 0.0625, (0, 0, 0), 0.25)), dims=(1024, 1024, 1024), offset=(1 << 20, -(1 << 20), 0), **big)
    assert L.stub_window_count() == 2
    # the host-only twin says the same of the spec, on a line of its own
    out = c_volume(c.v)
    for offset, dims in ((((1 << 20) + 1, 0, 0), (4, 4, 4)), ((0, 0, 0), (0, 4, 4))):
        capfd.readouterr()
        assert not L.sgm_volume_window_spec(C.byref(c_volume(c.v)), int3(offset), int3(dims), C.byref(out))
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("sgm_mi355x: sgm_volume_window_spec: ") and bytes(out) == bytes(c_volume(c.v))
    L.sgm_destroy(s)


def test_host_without_the_launcher_links_and_refuses(host_without, capfd):
    L = host_without
    s = L.sgm_create(0)
    c = Call(L, s)
    L.stub_clear()
    capfd.readouterr()
    assert not c()
    err = capfd.readouterr().err
    assert err.startswith("sgm_mi355x: sgm_volume_window: ") and err.endswith("not part of this build\n") and err.count("\n") == 1, err
    assert standin.log(L) == [] and all(h.untouched() for h in c.all)
    out = c_volume(c.v)                                           # the host-only calls need no launcher
    assert L.sgm_volume_window_spec(C.byref(c_volume(c.v)), int3((4, -3, 2)), int3((5, 6, 7)), C.byref(out)) and (out.nx, out.ny, out.nz) == (5, 6, 7)
    L.sgm_destroy(s)


W, H = 48, 20


def test_plain_match_logs_what_it_logs_without_the_window(host, host_without):
    """allocations and their sizes included: an instance that never calls the entry point is the instance it was"""
    import soc_project_stereo_matching_amd as S
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs = []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                                           conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        L.sgm_destroy(s)
    assert logs[0] == logs[1] and len(logs[0]) > 10
    host.stub_window_clear()
    assert host.stub_window_count() == 0


def test_a_refused_launch_or_wait_fails_the_call_and_the_call_waits_for_a_match_in_flight(host):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    opt = S.default_option(16)
    c = Call(L, s)
    clear(L)
    L.stub_window_fail_at(0)
    assert not c() and L.stub_window_count() == 1 and c.untouched()   # the spec is handed out only with the launch
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    clear(L)
    assert c()
    assert "wait_event" in [e.name for e in standin.log(L)] and "alloc" not in [e.name for e in standin.log(L)]
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    clear(L)
    L.stub_fail_at(b"wait_event", 0)
    assert not c() and L.stub_window_count() == 0
    assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- the driver on the stand-in ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("window_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"), STUB_VOLUME, STUB_RAYCAST, STUB_MESH,
                                        STUB_COLOR, STUB_WINDOW], libs=("-lz",))


def test_driver_on_the_stand_in_writes_the_window_and_without_the_flag_what_it_wrote(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75"""
    from test_driver_mesh import WIDE, read_mesh_ply, spec_of
    from test_driver_volume import PIN, write_pgm
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, mesh, plain_mesh, color_mesh = (str(tmp_path / n) for n in ("d.f32", "v.ply", "m.ply", "pm.ply", "cm.ply"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN)]
    for extra, says in ((["--volume-window", "4,-2,1,32,20,8"], "--volume-window needs --volume"),
                        (["--volume", WIDE, "--volume-ply", ply, "--volume-window", "4,-2,1,32,20"], "--volume-window wants OX,OY,OZ,NX,NY,NZ")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    offset, dims = (4, -2, 1), (32, 20, 8)
    window = ",".join(str(x) for x in offset + dims)
    base += ["--volume-ply", ply]
    out = subprocess.run(base + ["--volume", WIDE, "--volume-mesh", plain_mesh], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "volume window" not in out.stdout, (out.stdout[-500:], out.stderr[-500:])
    out = subprocess.run(base + ["--volume", WIDE, "--volume-mesh", mesh, "--volume-window", window], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    assert "volume window: 32 x 20 x 8 voxels from (4, -2, 1), origin (-42, -33, 44.5)" in out.stdout
    v = spec_of(WIDE)
    fx, fy, cx, cy, baseline, doffs = (float(x) for x in PIN)
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs)
    disp = np.fromfile(raw, np.float32).reshape(1, h, w)
    vox, col, _ = KR.integrate(VR.empty(v), KR.empty(v), v, s, VR.pose()[None], disp, None, None, img.reshape(1, h, w), 1)
    wv, wvox, wcol = WR.window_spec(v, offset, dims), WR.window(vox, v, offset, dims), WR.window(col, v, offset, dims)
    assert wv.origin == (-42.0, -33.0, 44.5)
    # without the flag: the whole volume's mesh, as before;  with it: the window's
    for path, (vert, tri) in ((plain_mesh, MR.mesh(vox, v, 1)), (mesh, MR.mesh(wvox, wv, 1))):
        xyz, faces = read_mesh_ply(path)
        assert xyz.tobytes() == np.stack([vert["x"], vert["y"], vert["z"]], axis=1).tobytes() and np.array_equal(faces, tri["v"]) and len(tri) > 300
    assert f"volume: {(wvox >> 16 != 0).sum()} of {wvox.size} voxels seen, {len(VR.crossings(wvox, wv, 1))} surface points" in out.stdout
    # with colours: both arrays are windowed
    out = subprocess.run(base + ["--volume", WIDE, "--volume-mesh", color_mesh, "--volume-color", "--volume-window", window], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vert, tri = MR.mesh(wvox, wv, 1)
    body = open(color_mesh, "rb").read().split(b"end_header\n", 1)[1]
    got = np.frombuffer(body[:15 * len(vert)], np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]))
    want = KR.colors(wvox, wcol, wv, vert["id"], 8)
    assert len(body) == 15 * len(vert) + 13 * len(tri) and got["xyz"].tobytes() == np.stack([vert["x"], vert["y"], vert["z"]], axis=1).tobytes()
    assert np.array_equal(got["rgb"], np.stack([want & 0xFF, (want >> 8) & 0xFF, (want >> 16) & 0xFF], axis=1).astype(np.uint8))
    assert (want >> 24 == 0xFF).sum() > 0.9 * len(vert)
    # a window the library refuses fails the run
    out = subprocess.run(base + ["--volume", WIDE, "--volume-window", "0,0,0,0,4,4"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "sgm_mi355x: sgm_volume_window_spec: " in out.stderr


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_window_host_is_asan_ubsan_clean(tmp_path):
    """tests/window_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in launcher."""
    exe = standin.build(tmp_path, sanitize=True, exe="window_sanitize_driver", flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "window_sanitize_driver.c"), STUB_WINDOW])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("window_sanitize_driver ok")


# ---- the kernel's resources ----------------------------------------------------------------------------------------------------

def test_the_kernel_compiles_without_lds_scratch_or_spills_and_the_committed_table_is_this_builds(tmp_path):
    """the compile-time gate: no LDS, 0 bytes of scratch and no spills in all six instantiations, and
    profiles/volume_window_resources.txt records this build"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", fh.read(), re.M | re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sgm_window.hip"),
                          "-o", str(tmp_path / "sgm_window.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for block in out.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z\d+sgm_volume_window_kILi(\d)ELb([01])ELb([01])EE", block.split()[0])
        assert m, block.split()[0]
        num = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))
        name = "sgm_volume_window_k<%s,%s,%s>" % (m.group(1), "true" if m.group(2) == "1" else "false", "true" if m.group(3) == "1" else "false")
        got[name] = [num(r"TotalSGPRs"), num(r" VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"),
                     num(r"Occupancy \[waves/SIMD\]"), num(r"SGPRs Spill"), num(r"VGPRs Spill")]
    assert sorted(got) == sorted("sgm_volume_window_k<%s,%s>" % (va, c) for va in ("4,true", "4,false", "1,false") for c in ("true", "false")), got
    for name, (sgpr, vgpr, scratch, lds, occ, s_spill, v_spill) in got.items():
        assert scratch == 0 and lds == 0 and s_spill == 0 and v_spill == 0, (name, got[name])
    with open(os.path.join(ROOT, "profiles", "volume_window_resources.txt")) as fh:
        rows = [ln.split() for ln in fh.read().splitlines() if ln.startswith("sgm_volume_window_k<")]
    # kernel | SGPR VGPR scratch LDS occ. spills
    table = {r[0]: [int(x) for x in r[2:7]] + [int(x) for x in r[7].split("+")] for r in rows}
    assert table == got


def test_the_bounded_grid_is_named_where_the_large_tests_read_it():
    from geometry_large import constant
    assert constant("sgm_window.hip", "WIN_THREADS") % 64 == 0 and constant("sgm_window.hip", "WIN_MAX_BLOCKS") >= 1
