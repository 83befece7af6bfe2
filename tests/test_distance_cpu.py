"""The distance field of the TSDF volume (extension; the contract is the distance section of include/sgm_mi355x.h) without a GPU: the
numpy restatement tests/distance_ref.py against brute force (and scipy where it imports), the rim of the radius, an analytic ball,
the sign, composition with the window, a fused scene, header / library / Python agreement, the C host's logic and the driver on the
stand-in device (tests/stub_device.c + stub_distance.c), a sanitizer run of a stand-alone driver, and the kernels' compile-time
resources.  Tolerance 0: words and bytes are compared; the one bound is the ball's, which is analytic."""
import ctypes as C
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import distance_ref as DR
import standin
import volume_ref as VR
import window_ref as WR
from conftest import ROOT
from test_color_cpu import STUB_COLOR, STUB_MESH, Held
from test_raycast_cpu import STUB_RAYCAST
from test_volume_cpu import STUB_VOLUME, DeviceVolume, VOLUME_REFUSALS, bad_volume, c_volume, camera, noisy_maps
from test_window_cpu import STUB_WINDOW, sphere_scene

STUB_DISTANCE = os.path.join(ROOT, "tests", "stub_distance.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
FAR = DR.FAR

# ---- cases (shared with tests/test_gpu_volume_distance.py) ---------------------------------------------------------------------

SMALL_DIMS = [(1, 1, 1), (17, 1, 1), (1, 17, 1), (1, 1, 17), (5, 3, 2), (13, 5, 3), (12, 11, 10)]
DENSITIES = (0.0, 0.01, 0.2, 1.0)


def planted_words(rng, dims, density, min_weight):
    """uint32 [nz][ny][nx]: about `density` of the voxels occupied (observed at min_weight, tq < 0), the others unobserved or observed
    and free (tq >= 0, zero among them) in equal parts, random bits otherwise; the word 0 among them, and 0xFFFFFFFF where any voxel
    is occupied"""
    shape = (dims[2], dims[1], dims[0])
    occupied = rng.random(shape) < density
    observed = occupied | (rng.random(shape) < 0.5)
    w = np.where(observed, rng.integers(min_weight, 65536, shape), rng.integers(0, min_weight, shape)).astype(np.uint32)
    tq = np.where(occupied, rng.integers(-32768, 0, shape), rng.integers(0, 32768, shape)).astype(np.int16)
    tq = np.where(~occupied & (rng.random(shape) < 0.1), 0, tq).astype(np.int16)
    words = (w << 16) | tq.view(np.uint16).astype(np.uint32)
    flat = words.reshape(-1)
    if density < 1.0:
        flat[flat.size // 2] = 0
    if density > 0.0:
        flat[flat.size // 3] = 0xFFFFFFFF
    return words


def one_site(dims, at, min_weight=1):
    """every voxel observed and free but the one at (i, j, k)"""
    words = np.full((dims[2], dims[1], dims[0]), (min_weight << 16) | 5, np.uint32)
    words[at[2], at[1], at[0]] = (min_weight << 16) | 0x8000
    return words


RIM = (((3, 4, 0), 25), ((0, 0, 5), 25), ((5, 1, 0), FAR), ((4, 3, 1), FAR))


def rim_cases():
    """(words, the site, [(the voxel, the word it must hold)]): one site in the middle of 13^3 and in each corner, r = 5"""
    n = 13
    for site in [(6, 6, 6)] + list(itertools.product((0, n - 1), repeat=3)):
        sign = [1 if c < n - 1 else -1 for c in site]
        checks = []
        for off, want in RIM:
            for perm in set(itertools.permutations(off)):
                checks.append((tuple(c + s * o for c, s, o in zip(site, sign, perm)), want))
        yield one_site((n, n, n), site), site, checks


def check_rim(result, site, checks):
    assert result[site[2], site[1], site[0]] == 0
    for (i, j, k), want in checks:
        assert result[k, j, i] == want, (site, (i, j, k), int(result[k, j, i]), want)


@functools.lru_cache(maxsize=None)
def fused_scene():
    """(v, s, poses, disp, words0, fused): the sphere of tests/test_window_cpu.py with one noisy frame fused into it by volume_ref,
    seen from a camera placed in front of its box"""
    v, words0 = sphere_scene()
    s = camera(70, 33, frames=1)
    poses = VR.pose(np.eye(3), (0.5, -1.03, -1.3))[None]
    disp = noisy_maps(s, np.random.default_rng(41), non_finite=False)
    fused = VR.integrate(words0, v, s, poses, disp)[0]
    fused.setflags(write=False)
    return v, s, poses, disp, words0, fused


@functools.lru_cache(maxsize=None)
def fused_reference(min_weight=1, r=6):
    """(side 0, side 1, the signed field, the unsigned field) of the fused scene"""
    v, *_, fused = fused_scene()
    o, i = DR.distance(fused, min_weight, r, 0, 0), DR.distance(fused, min_weight, r, 1, 0)
    return o, i, DR.field(o, i, v.voxel), DR.field(o, None, v.voxel)


# ---- the restatement against brute force ---------------------------------------------------------------------------------------

def brute(site, r):
    """the minimum over all sites, computed directly"""
    nz, ny, nx = site.shape
    out = np.full(site.shape, FAR, np.uint16)
    K, J, I = np.nonzero(site)
    if len(K) == 0:
        return out
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = ((kk[..., None] - K) ** 2 + (jj[..., None] - J) ** 2 + (ii[..., None] - I) ** 2).min(axis=-1)
    out[d <= r * r] = d[d <= r * r]
    return out


def small_cases():
    """(dims, density, min_weight, words) of the list both suites run"""
    for n, dims in enumerate(SMALL_DIMS):
        for m, density in enumerate(DENSITIES):
            min_weight = (1, 9)[(n + m) % 2]
            yield dims, density, min_weight, planted_words(np.random.default_rng(1000 + 10 * n + m), dims, density, min_weight)


def test_restatement_equals_brute_force():
    seen = set()
    for dims, density, min_weight, words in small_cases():
        for side in (0, 1):
            for unknown in (0, 1):
                site = DR.sites(words, min_weight, side, unknown)
                seen.add((bool(site.any()), bool(site.all())))
                for r in (1, 2, 3, 5, 255):
                    got = DR.distance(words, min_weight, r, side, unknown)
                    assert got.dtype == np.uint16 and np.array_equal(got, brute(site, r)), (dims, density, side, unknown, r)
                    assert np.all(got[site] == 0) and np.all(got[~site] != 0)
    assert seen == {(False, False), (True, False), (True, True)}
    # the predicate, word by word: zero counts as non-negative, the weight is compared, not tested for zero
    words = np.array([[[0x00000000, 0x00010000, 0x00018000, 0x0001FFFF, 0x00087FFF, 0x00098000, 0xFFFFFFFF, 0x0008FFFF]]], np.uint32)
    assert DR.obstacles(words, 1, 0).tolist() == [[[False, False, True, True, False, True, True, True]]]
    assert DR.obstacles(words, 9, 0).tolist() == [[[False, False, False, False, False, True, True, False]]]
    assert DR.obstacles(words, 9, 1).tolist() == [[[True, True, True, True, True, True, True, True]]]
    assert DR.sites(words, 9, 1, 0).tolist() == [[[True, True, True, True, True, False, False, True]]]


def test_restatement_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for dims, density, min_weight, words in small_cases():
        for side, unknown in ((0, 0), (1, 0), (0, 1), (1, 1)):
            site = DR.sites(words, min_weight, side, unknown)
            for r in (1, 2, 3, 5, 255):
                want = np.full(site.shape, FAR, np.uint16)
                if site.any():
                    d = ndimage.distance_transform_edt(~site)
                    d2 = np.rint(d * d).astype(np.int64)
                    want = np.where(d2 <= r * r, d2, FAR).astype(np.uint16)
                assert np.array_equal(DR.transform(site, r), want), (dims, density, side, unknown, r)


def test_the_rim_of_the_radius_in_the_middle_and_in_every_corner():
    count = 0
    for words, site, checks in rim_cases():
        assert len(checks) == 6 + 3 + 6 + 6
        check_rim(DR.distance(words, 1, 5), site, checks)
        count += 1
    assert count == 9


def ball_scene(n=32, rho=6.0, min_weight=1):
    """(words, c): voxels whose centres lie within rho voxels of the middle of n^3 occupied, the rest observed and free; c: the
    distance of every centre from the middle, in voxels"""
    axis = np.arange(n) + 0.5 - n / 2.0
    c = np.sqrt(axis[:, None, None] ** 2 + axis[None, :, None] ** 2 + axis[None, None, :] ** 2)
    words = np.where(c <= rho, (min_weight << 16) | 0xC000, (min_weight << 16) | 0x4000).astype(np.uint32)
    return words, c


def check_ball(o, i, f, c, rho, r, voxel):
    """Outside, at centre distance c: a lattice point within sqrt(3)/2 of the point sqrt(3)/2 inside the ball on the ray to the
    middle always exists and lies in the ball, so the distance to the nearest occupied centre is in [c - rho, c - rho + sqrt(3)].
    Inside likewise against the free voxels: [rho - c, rho - c + sqrt(3)] (the nearest free centre is beyond rho).  Widened by
    4 ulps of the value for the float32 square root and product."""
    inside = c <= rho
    eps = 4 * np.finfo(np.float32).eps
    lo_out, hi_out = voxel * (c - rho), voxel * (c - rho + np.sqrt(3.0))
    near = ~inside & (o != FAR)
    assert near.sum() > 1000 and np.all(o[~inside & (c - rho + np.sqrt(3.0) <= r)] != FAR)
    assert np.all(f[near] >= lo_out[near] * (1 - eps)) and np.all(f[near] <= hi_out[near] * (1 + eps))
    assert np.all(np.isposinf(f[~inside & (o == FAR)])) and np.all(c[~inside & (o == FAR)] - rho > r - np.sqrt(3.0))
    assert inside.sum() > 500 and np.all(f[inside] < 0) and np.all(o[inside] == 0) and np.all(i[inside] != FAR)
    mag = -f[inside].astype(np.float64)
    assert np.all(mag >= voxel * (rho - c[inside]) * (1 - eps)) and np.all(mag <= voxel * (rho - c[inside] + np.sqrt(3.0)) * (1 + eps))


def test_an_analytic_ball():
    words, c = ball_scene()
    voxel, r, rho = 0.0625, 9, 6.0
    o, i = DR.distance(words, 1, r, 0, 0), DR.distance(words, 1, r, 1, 0)
    check_ball(o, i, DR.field(o, i, voxel), c, rho, r, voxel)


def test_the_sign_is_membership_in_the_obstacle_set():
    for dims, density, min_weight, words in small_cases():
        for unknown in (0, 1):
            o, i = DR.distance(words, min_weight, 3, 0, unknown), DR.distance(words, min_weight, 3, 1, unknown)
            in_o = DR.obstacles(words, min_weight, unknown)
            assert not np.any((o == 0) & (i == 0)) and np.array_equal(o == 0, in_o) and np.array_equal(i == 0, ~in_o)
            f = DR.field(o, i, 0.05)
            assert f.dtype == np.float32 and np.array_equal(f < 0, in_o) and np.all(f[~in_o] > 0) and np.array_equal(np.signbit(f), in_o)
    # the field, word by word
    words16 = np.array([0, 1, 2, 65025, FAR], np.uint16)
    o, i = np.meshgrid(words16, words16, indexing="ij")
    f, v = DR.field(o, i, 0.05), np.float32(0.05)
    assert np.all(np.isposinf(f[4])) and f[1, 0] == v and f[3, 2] == v * np.float32(255.0) and f[2, 4] == v * np.sqrt(np.float32(2.0))
    assert f[0, 0] == 0 and not np.signbit(f[0, 0]) and np.isneginf(f[0, 4]) and f[0, 1] == -v and f[0, 3] == -(v * np.float32(255.0))
    assert np.array_equal(DR.field(o, None, 0.05)[0], np.zeros(5, np.float32)) and not np.any(np.signbit(DR.field(o, None, 0.05)[0]))


def test_a_window_with_a_margin_of_r_gives_the_sources_distances():
    rng = np.random.default_rng(77)
    dims, r = (24, 19, 15), 4
    src = VR.spec(*dims, 0.0625, (-1.125, -1.0, 0.5), 0.25)
    words = planted_words(rng, dims, 0.02, 1)
    lo, n = (7, 6, 5), (6, 5, 4)                                   # the box, in the source
    offset, wdims = tuple(c - r for c in lo), tuple(m + 2 * r for m in n)
    win = WR.window(words, src, offset, wdims)
    for side, unknown in ((0, 0), (1, 0), (0, 1)):
        whole = DR.distance(words, 1, r, side, unknown)
        part = DR.distance(win, 1, r, side, unknown)
        box = whole[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]]
        assert np.array_equal(part[r:r + n[2], r:r + n[1], r:r + n[0]], box), (side, unknown)
        assert (box != FAR).any() and (box != 0).any()
    # one voxel less of margin is not enough: a site just outside the window changes a word on the box's face
    words2 = one_site(dims, (lo[0] - r, lo[1], lo[2]))
    tight = WR.window(words2, src, (offset[0] + 1, offset[1], offset[2]), wdims)
    assert DR.distance(words2, 1, r)[lo[2], lo[1], lo[0]] == r * r and DR.distance(tight, 1, r)[r, r, r - 1] == FAR


def test_a_fused_scene_through_both_sides_and_the_field():
    v, s, poses, disp, words0, fused = fused_scene()
    assert (fused != words0).sum() > 500
    o, i, f, u = fused_reference()
    assert np.array_equal(o, brute(DR.sites(fused, 1, 0, 0), 6)) and np.array_equal(i, brute(DR.sites(fused, 1, 1, 0), 6))
    assert (o == 0).sum() > 300 and (o == FAR).sum() > 100 and ((o != 0) & (o != FAR)).sum() > 1000 and (f < 0).sum() == (o == 0).sum()
    assert np.array_equal(u[o != 0], f[o != 0]) and np.all(u[o == 0] == 0)
    assert not np.array_equal(o, DR.distance(words0, 1, 6, 0, 0))           # the frame changed the obstacle set


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


ENTRIES = ("sgm_volume_distance_bytes", "sgm_volume_distance", "sgm_volume_distance_field")


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name), name
    assert hasattr(lib, "sgmd_volume_distance") and hasattr(lib, "sgmd_volume_distance_field")
    assert callable(getattr(S.SGMInstance, "volume_distance", None)) and callable(getattr(S.SGMInstance, "volume_distance_field", None))
    for name in ("SGMDistanceSpec", "DISTANCE_FAR", "distance_spec", "volume_distance_bytes"):
        assert name in S.__all__ and hasattr(S, name), name
    assert C.sizeof(S.SGMDistanceSpec) == 16 and [(n, getattr(S.SGMDistanceSpec, n).offset) for n, _ in S.SGMDistanceSpec._fields_] == \
        [("min_weight", 0), ("radius", 4), ("side", 8), ("unknown", 12)]
    d = S.distance_spec(9, 255)
    assert (d.min_weight, d.radius, d.side, d.unknown) == (9, 255, 0, 0) and S.DISTANCE_FAR == FAR == 0xFFFF
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    assert re.search(r"^#define SGM_DISTANCE_FAR 0xFFFFu$", text, re.M)
    head = "the distance field of the TSDF volume: the exact Euclidean distance transform of its voxel lattice"
    assert text.count(head) == 1 and text.index(head) > text.index("int  sgm_volume_leaving(")
    block = text.split(head)[1].split("size_t sgm_volume_distance_bytes")[0]
    for line in ("observed    w >= min_weight", "occupied    observed and tq < 0", "m = min over sites q of (pi-qi)^2 + (pj-qj)^2 + (pk-qk)^2",
                 "otherwise SGM_DISTANCE_FAR; a site gets 0", "out[j] = min over |o| <= r of g[j+o] + o*o", "no instance scratch and",
                 "spec->voxel * sqrtf((float)o)", "-(spec->voxel * sqrtf((float)i))", "half a voxel", "Not part of it:", "incremental update",
                 "the identity of the nearest site", "a radius above 255", "2-D", "queries at arbitrary points", "16 bytes, every field 4 bytes, no padding"):
        assert line in block, line
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "sgm_host.c")) as fh:
        host = fh.read()
    assert "#pragma weak sgmd_volume_distance\n" in host and "#pragma weak sgmd_volume_distance_field\n" in host
    with open(os.path.join(csrc, "Makefile")) as fh:
        assert re.search(r"^HIP_UNITS := .*\bsgm_distance\b", fh.read(), re.M)
    v = sphere_scene()[0]
    assert S.volume_distance_bytes(c_volume(v)) == 2 * v.nx * v.ny * v.nz == S.volume_bytes(c_volume(v)) // 2
    assert S.volume_distance_bytes(c_volume(bad_volume(nx=0))) == 0
    assert S.volume_distance_bytes(c_volume(VR.spec(1024, 1024, 1024, 0.0625, (0, 0, 0), 0.25))) == 1 << 31


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

class DistanceSpec(C.Structure):
    _fields_ = [("min_weight", C.c_uint32), ("radius", C.c_int32), ("side", C.c_int32), ("unknown", C.c_int32)]


def _sign(L):
    for name, (res, args) in {"sgm_volume_distance": (_b, [_p] * 5), "sgm_volume_distance_field": (_b, [_p] * 5),
                              "sgm_volume_distance_bytes": (_z, [_p]), "stub_distance_clear": (None, []), "stub_distance_count": (_i, []),
                              "stub_distance_kind": (_i, [_i]), "stub_distance_ptr": (_p, [_i, _i]), "stub_distance_int": (_i, [_i, _i]),
                              "stub_distance_volume": (C.POINTER(DeviceVolume), [_i]), "stub_distance_fail_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("distancestub"), extra_sources=[STUB_DISTANCE], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("distancestub_without"), flags=("-ffp-contract=off",)))


class Call:
    """the arrays of the two calls on the fused scene, and the calls with any argument replaced.  Held counts 32-bit words: the
    16-bit arrays take half as many, and an odd count is rounded up into the pad."""
    def __init__(self, L, s):
        self.L, self.s = L, s
        self.v, _, _, _, _, self.fused = fused_scene()
        self.n = self.fused.size
        assert self.n % 2 == 0
        o, i, _, _ = fused_reference()
        self.vox, self.dist = Held(self.n, self.fused), Held(self.n // 2)
        self.o, self.i, self.field = Held(self.n // 2, o.view(np.uint32)), Held(self.n // 2, i.view(np.uint32)), Held(self.n)
        self.all = (self.vox, self.dist, self.o, self.i, self.field)

    def untouched(self):
        return all(h.untouched() for h in self.all)

    def distance(self, **kw):
        a = dict(s=self.s, spec=c_volume(self.v), dist=DistanceSpec(1, 6, 0, 0), vox=self.vox.ptr, out=self.dist.ptr)
        a.update(kw)
        ref = lambda t: None if t is None else C.byref(t)
        return self.L.sgm_volume_distance(a["s"], ref(a["spec"]), ref(a["dist"]), a["vox"], a["out"])

    def to_field(self, **kw):
        a = dict(s=self.s, spec=c_volume(self.v), o=self.o.ptr, i=self.i.ptr, field=self.field.ptr)
        a.update(kw)
        return self.L.sgm_volume_distance_field(a["s"], None if a["spec"] is None else C.byref(a["spec"]), a["o"], a["i"], a["field"])


def clear(L):
    L.stub_clear(); L.stub_distance_clear()


def test_the_validated_specs_and_the_callers_pointers_arrive_and_the_stand_in_equals_the_restatement(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: the distance field needs no shape
    c = Call(L, s)
    o, i, f, u = fused_reference()
    for side, unknown, min_weight, r in ((0, 0, 1, 6), (1, 0, 1, 6), (0, 1, 2, 3), (1, 1, 65535, 255), (0, 0, 1, 1)):
        c = Call(L, s)
        clear(L)
        assert c.distance(dist=DistanceSpec(min_weight, r, side, unknown))
        assert L.stub_distance_count() == 1 and standin.log(L) == []  # no allocation, no copy, no wait without a match in flight
        assert L.stub_distance_kind(0) == 0 and [L.stub_distance_ptr(0, k) for k in range(3)] == [c.vox.ptr, c.dist.ptr, None]
        assert [L.stub_distance_int(0, k) for k in range(4)] == [min_weight, r, side, unknown]
        assert bytes(L.stub_distance_volume(0).contents) == bytes(c_volume(c.v))
        assert np.array_equal(c.dist.words().view(np.uint16), DR.distance(c.fused, min_weight, r, side, unknown).reshape(-1)), (side, unknown, r)
        assert c.vox.untouched() and c.field.untouched()
    for signed in (True, False):
        c = Call(L, s)
        clear(L)
        assert c.to_field() if signed else c.to_field(i=None)
        assert L.stub_distance_count() == 1 and standin.log(L) == [] and L.stub_distance_kind(0) == 1
        assert [L.stub_distance_ptr(0, k) for k in range(3)] == [c.o.ptr, c.i.ptr if signed else None, c.field.ptr]
        assert bytes(L.stub_distance_volume(0).contents) == bytes(c_volume(c.v))
        assert c.field.words().view(np.float32).tobytes() == (f if signed else u).tobytes()
        assert c.o.untouched() and c.i.untouched() and c.vox.untouched() and c.dist.untouched()
    L.sgm_destroy(s)


def refused(c, call, entry, capfd, **kw):
    """false, one line on stderr that names the entry point, nothing logged, nothing touched"""
    clear(c.L)
    capfd.readouterr()
    assert not call(**kw), kw
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("sgm_mi355x: %s: " % entry), (kw, err)
    assert c.L.stub_distance_count() == 0 and standin.log(c.L) == []
    assert c.untouched(), kw
    return err


def test_every_refusal_queues_nothing_and_prints_its_line(host, capfd):
    L = host
    s = L.sgm_create(0)
    c = Call(L, s)
    d = lambda **kw: refused(c, c.distance, "sgm_volume_distance", capfd, **kw)
    f = lambda **kw: refused(c, c.to_field, "sgm_volume_distance_field", capfd, **kw)
    for kw in (dict(s=None), dict(spec=None), dict(dist=None), dict(vox=None), dict(out=None)):
        assert "NULL argument" in d(**kw)
    for kw in (dict(s=None), dict(spec=None), dict(o=None), dict(field=None)):
        assert "NULL argument" in f(**kw)
    for name, bad in sorted(VOLUME_REFUSALS.items()):
        assert "outside its ranges" in d(spec=c_volume(bad_volume(**bad))), name
        assert "outside its ranges" in f(spec=c_volume(bad_volume(**bad))), name
    for mw in (0, 65536, 0xFFFFFFFF):
        assert "min_weight" in d(dist=DistanceSpec(mw, 6, 0, 0)), mw
    for r in (0, -1, 256, 1 << 30, -(1 << 31)):
        assert "radius" in d(dist=DistanceSpec(1, r, 0, 0)), r
    for side, unknown in ((2, 0), (-1, 0), (0, 2), (0, -1), (1 << 30, 1)):
        assert "0 or 1" in d(dist=DistanceSpec(1, 6, side, unknown)), (side, unknown)
    assert "not aligned" in d(vox=c.vox.ptr + 2) and "not aligned" in d(vox=c.vox.ptr + 1) and "not aligned" in d(out=c.dist.ptr + 1)
    for kw in (dict(o=c.o.ptr + 1), dict(i=c.i.ptr + 1), dict(field=c.field.ptr + 2), dict(field=c.field.ptr + 1)):
        assert "not aligned" in f(**kw), kw
    nb = 4 * c.n
    x = c.vox.ptr
    for kw in (dict(out=x), dict(out=x + nb - 2), dict(out=x - nb // 2 + 2), dict(vox=c.dist.ptr), dict(vox=c.dist.ptr - nb + 4)):
        assert "overlaps" in d(**kw), kw
    a, b, g = c.o.ptr, c.i.ptr, c.field.ptr
    for kw in (dict(field=a), dict(field=a + nb // 2 - 4), dict(field=a - nb + 4), dict(field=b), dict(field=b - nb + 4), dict(o=g + 8), dict(i=g + nb - 2)):
        assert "overlaps" in f(**kw), kw
    # allowed: arrays that touch, the two sides one and the same array, 2-byte alignment of the words, the largest volume and the
    # ends of every range (the stand-in only logs a volume beyond 1 MiB)
    clear(L)
    one = np.full(c.n + c.n // 2, 0xA5A5A5A5, np.uint32)          # the volume | the distances
    one[:c.n] = c.fused.reshape(-1)
    assert c.distance(vox=one.ctypes.data, out=one.ctypes.data + nb) and L.stub_distance_count() == 1
    assert np.array_equal(one[c.n:].view(np.uint16), fused_reference()[0].reshape(-1)) and np.array_equal(one[:c.n], c.fused.reshape(-1))
    assert c.to_field(i=a) and L.stub_distance_count() == 2
    big = c_volume(VR.spec(1024, 1024, 1024, 0.0625, (0, 0, 0), 0.25))
    assert c.distance(spec=big, dist=DistanceSpec(65535, 255, 1, 1), vox=1 << 44, out=(1 << 45) + 2)
    assert c.to_field(spec=big, o=(1 << 44) + 2, i=(1 << 45) + 6, field=(1 << 46) + 4) and L.stub_distance_count() == 4
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_without, capfd):
    L = host_without
    s = L.sgm_create(0)
    c = Call(L, s)
    for call, entry in ((c.distance, "sgm_volume_distance"), (c.to_field, "sgm_volume_distance_field")):
        L.stub_clear()
        capfd.readouterr()
        assert not call()
        err = capfd.readouterr().err
        assert err.startswith("sgm_mi355x: %s: " % entry) and err.endswith("not part of this build\n") and err.count("\n") == 1, err
        assert standin.log(L) == [] and c.untouched()
    assert L.sgm_volume_distance_bytes(C.byref(c_volume(c.v))) == 2 * c.n     # the host-only call needs no launcher
    L.sgm_destroy(s)


W, H = 48, 20


def test_plain_match_logs_what_it_logs_without_the_distance_field(host, host_without):
    """allocations and their sizes included: an instance that never calls the entry points is the instance it was"""
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
    host.stub_distance_clear()
    assert host.stub_distance_count() == 0


def test_a_refused_launch_or_wait_fails_the_call_and_the_call_waits_for_a_match_in_flight(host):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    opt = S.default_option(16)
    c = Call(L, s)
    for call in (c.distance, c.to_field):
        clear(L)
        L.stub_distance_fail_at(0)
        assert not call() and L.stub_distance_count() == 1 and c.untouched()
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    for call in (c.distance, c.to_field):
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        clear(L)
        assert call()
        assert "wait_event" in [e.name for e in standin.log(L)] and "alloc" not in [e.name for e in standin.log(L)]
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        clear(L)
        L.stub_fail_at(b"wait_event", 0)
        assert not call() and L.stub_distance_count() == 0
        assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- the driver on the stand-in ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("distance_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"), STUB_VOLUME, STUB_RAYCAST, STUB_MESH,
                                        STUB_COLOR, STUB_WINDOW, STUB_DISTANCE], libs=("-lz",))


def read_field(path):
    raw = open(path, "rb").read()
    dims = np.frombuffer(raw[:12], np.int32)
    voxel = np.frombuffer(raw[12:16], np.float32)[0]
    body = np.frombuffer(raw[16:], np.float32)
    assert body.size == dims.prod()
    return tuple(int(x) for x in dims), voxel, body.reshape(dims[2], dims[1], dims[0])


def test_driver_on_the_stand_in_writes_the_field_and_without_the_flag_what_it_wrote(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75"""
    import cloud_ref as CR
    from test_driver_mesh import WIDE, spec_of
    from test_driver_volume import PIN, write_pgm
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, ply2, mesh, mesh2, field, wfield = (str(tmp_path / n) for n in ("d.f32", "v.ply", "v2.ply", "m.ply", "m2.ply", "f.f32", "wf.f32"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN)]
    for extra, says in ((["--volume-distance", "3", "--volume-field", field], "--volume-distance needs --volume"),
                        (["--volume", WIDE, "--volume-ply", ply, "--volume-distance", "3"], "--volume-distance and --volume-field OUT.f32 go together"),
                        (["--volume", WIDE, "--volume-ply", ply, "--volume-field", field], "--volume-distance and --volume-field OUT.f32 go together"),
                        (["--volume", WIDE, "--volume-ply", ply, "--volume-distance", "x", "--volume-field", field], "--volume-distance wants R[,UNKNOWN]")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    plain = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply, "--volume-mesh", mesh], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "volume field" not in plain.stdout, (plain.stdout[-500:], plain.stderr[-500:])
    out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-mesh", mesh2, "--volume-distance", "3", "--volume-field", field],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    # without the flag the driver writes what it wrote; with it, the other outputs are the same bytes and lines
    assert open(ply, "rb").read() == open(ply2, "rb").read() and open(mesh, "rb").read() == open(mesh2, "rb").read()
    said = lambda text: [ln for ln in text.splitlines() if not ln.startswith("volume field") and not re.search(r"\d ms\b", ln)]   # (times vary)
    assert said(out.stdout) == said(plain.stdout) and len(said(plain.stdout)) >= 3
    v = spec_of(WIDE)
    fx, fy, cx, cy, baseline, doffs = (float(x) for x in PIN)
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs)
    disp = np.fromfile(raw, np.float32).reshape(1, h, w)
    vox = VR.integrate(VR.empty(v), v, s, VR.pose()[None], disp)[0]

    def want(words, spec, r, unknown):
        o, i = DR.distance(words, 1, r, 0, unknown), DR.distance(words, 1, r, 1, unknown)
        return o, DR.field(o, i, spec.voxel)

    dims, voxel, got = read_field(field)
    o, f = want(vox, v, 3, 0)
    assert dims == (v.nx, v.ny, v.nz) and voxel == np.float32(v.voxel) and got.tobytes() == f.tobytes()
    assert (f < 0).sum() > 100 and np.isposinf(f).sum() > 100 and ((f > 0) & np.isfinite(f)).sum() > 100
    assert f"volume field: radius 3, unknown 0: {(o == 0).sum()} obstacle voxels, {((o != 0) & (o != FAR)).sum()} within the radius" in out.stdout
    # after --volume-window, with unknown space as an obstacle
    offset, wd = (4, -2, 1), (32, 20, 8)
    out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-window", ",".join(str(x) for x in offset + wd),
                                 "--volume-distance", "2,1", "--volume-field", wfield], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    wv, wvox = WR.window_spec(v, offset, wd), WR.window(vox, v, offset, wd)
    dims, voxel, got = read_field(wfield)
    assert dims == wd and got.tobytes() == want(wvox, wv, 2, 1)[1].tobytes() and np.isneginf(got).sum() > 100 and ((got < 0) & np.isfinite(got)).sum() > 100
    # a radius the library refuses fails the run
    out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-distance", "256", "--volume-field", field], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode != 0 and "sgm_mi355x: sgm_volume_distance: " in out.stderr


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_distance_host_is_asan_ubsan_clean(tmp_path):
    """tests/distance_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in launchers."""
    exe = standin.build(tmp_path, sanitize=True, exe="distance_sanitize_driver", flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "distance_sanitize_driver.c"), STUB_DISTANCE])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("distance_sanitize_driver ok")


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------

KERNELS = {r"_Z22sgm_distance_x_short_k": "sgm_distance_x_short_k", r"_Z16sgm_distance_x_kILi(\d)EE": "sgm_distance_x_k<%s>",
           r"_Z19sgm_distance_line_kILi(\d+)ELb([01])EE": "sgm_distance_line_k<%s,%s>", r"_Z20sgm_distance_field_kILi(\d)EE": "sgm_distance_field_k<%s>"}


def test_the_kernels_compile_without_scratch_or_spills_within_their_lds_and_the_committed_table_is_this_builds(tmp_path):
    """the compile-time gate: 0 bytes of scratch and no spills in all nine instantiations, static LDS as the launcher's tiles
    (2 bytes per element of DIST_TILE_SMALL / DIST_TILE_LARGE, at most 64 KB, no dynamic LDS; 128 bytes per row of the x pass), and
    profiles/volume_distance_resources.txt records this build"""
    from geometry_large import constant
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", fh.read(), re.M | re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sgm_distance.hip"),
                          "-o", str(tmp_path / "sgm_distance.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for block in out.stderr.split("Function Name: ")[1:]:
        name = None
        for pat, fmt in KERNELS.items():
            m = re.match(pat, block.split()[0])
            if m:
                name = fmt % tuple({"0": "false", "1": "true"}[g] if k == 1 else g for k, g in enumerate(m.groups())) if m.groups() else fmt
        assert name, block.split()[0]
        num = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))
        got[name] = [num(r"TotalSGPRs"), num(r" VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"),
                     num(r"Occupancy \[waves/SIMD\]"), num(r"SGPRs Spill"), num(r"VGPRs Spill")]
    small, large = constant("sgm_distance.hip", "DIST_TILE_SMALL"), constant("sgm_distance.hip", "DIST_TILE_LARGE")
    lds = {"sgm_distance_x_short_k": 0, "sgm_distance_x_k<4>": 128 * constant("sgm_distance.hip", "DIST_X_WAVES"),
           "sgm_distance_x_k<1>": 128 * constant("sgm_distance.hip", "DIST_X_WAVES"), "sgm_distance_field_k<4>": 0, "sgm_distance_field_k<1>": 0}
    lds.update({"sgm_distance_line_k<%d,%s>" % (t, vec): 2 * t for t in (small, large) for vec in ("true", "false")})
    assert sorted(got) == sorted(lds) and 2 * large <= 65536, got
    with open(os.path.join(csrc, "sgm_distance.hip")) as fh:
        assert "hipFuncSetAttribute" not in fh.read()             # every launch passes 0 bytes of dynamic LDS
    for name, (sgpr, vgpr, scratch, lds_bytes, occ, s_spill, v_spill) in got.items():
        assert scratch == 0 and s_spill == 0 and v_spill == 0 and lds_bytes == lds[name], (name, got[name])
    with open(os.path.join(ROOT, "profiles", "volume_distance_resources.txt")) as fh:
        rows = [ln.split() for ln in fh.read().splitlines() if ln.startswith("sgm_distance_") and " | " in ln]
    # kernel | SGPR VGPR scratch LDS occ. spills
    table = {r[0]: [int(x) for x in r[2:7]] + [int(x) for x in r[7].split("+")] for r in rows}
    assert table == got


def test_the_tiers_are_named_where_the_device_tests_read_them():
    from geometry_large import constant
    c = lambda name: constant("sgm_distance.hip", name)
    assert c("DIST_THREADS") == 64 * c("DIST_X_WAVES") and c("DIST_MAX_BLOCKS") >= 1 and c("DIST_ROW_WAVE") == 64
    lines = [c("DIST_LINE_" + t) for t in "ABCD"]
    assert lines == sorted(lines) and lines[-1] < 1024
    # the strip of every tier fits its tile: 256, 128, 64 | 64, 32 columns of the longest line of the tier
    assert 256 * lines[0] <= c("DIST_TILE_SMALL") and 128 * lines[1] <= c("DIST_TILE_SMALL") and 64 * lines[2] <= c("DIST_TILE_SMALL")
    assert 64 * lines[3] <= c("DIST_TILE_LARGE") and 32 * 1024 <= c("DIST_TILE_LARGE")
