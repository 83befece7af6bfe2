"""The TSDF volume as a triangle mesh (extension; the contract is in include/sgm_mi355x.h, sgm_volume_mesh) without a GPU: the numpy
restatement tests/mesh_ref.py against itself (planted spheres are closed surfaces of genus 0 with outward normals, the generated
table is the geometric rule, the axis vertices are the surface points of tests/volume_ref.py), header / library / Python agreement,
the C host's logic on the stand-in device (tests/stub_device.c + tests/stub_mesh.c, which computes for real from the midpoint rule)
and a sanitizer run of a stand-alone driver.  Tolerance 0 wherever the library or the stand-in is compared with the restatement."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_ref as MR
import standin
import volume_ref as VR
from conftest import ROOT

STUB_MESH = os.path.join(ROOT, "tests", "stub_mesh.c")
STUB_VOLUME = os.path.join(ROOT, "tests", "stub_volume.c")
_p, _i, _b, _z, _u = C.c_void_p, C.c_int, C.c_bool, C.c_size_t, C.c_uint32
A5 = 0xA5A5A5A5
SPHERES = [(12, 11, 10), (9, 13, 7)]


def mesh_table():
    spec = importlib.util.spec_from_file_location("mesh_table", os.path.join(ROOT, "tools", "mesh_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_volume(dims, seed, weights=True, border=False, heavy=False):
    """random signs and magnitudes, zeros among them; random weights 0..2 (heavy: nine in ten are 2), or all 1; optionally a positive
    border"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    tq = rng.integers(-5, 6, size=(nz, ny, nx))
    if border:
        tq[0] = tq[-1] = 5
        tq[:, 0] = tq[:, -1] = 5
        tq[:, :, 0] = tq[:, :, -1] = 5
    w = rng.integers(0, 3, size=tq.shape) if weights else np.ones_like(tq)
    if heavy:
        w[rng.random(tq.shape) < 0.9] = 2
    return VR.spec(nx, ny, nz, 0.07, (0.5, -1.0, 2.0), 0.2), VR.pack(tq, w)


def same_mesh(label, got, want):
    (gv, gt), (wv, wt) = got, want
    assert len(gv) == len(wv) and len(gt) == len(wt), f"{label}: {len(gv)} vertices and {len(gt)} triangles, the restatement has {len(wv)} and {len(wt)}"
    assert gv.tobytes() == wv.tobytes(), f"{label}: the vertex list differs"
    assert gt.tobytes() == wt.tobytes(), f"{label}: the triangle list differs"


# ---- the restatement against itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SPHERES)
@pytest.mark.parametrize("zero_below", [0, 9000])
def test_planted_spheres_are_closed_genus_0_and_wound_outwards(dims, zero_below):
    v, vox = MR.sphere(dims, zero_below)
    vert, tri = MR.mesh(vox, v, 1)
    assert len(tri) > 150 and MR.closed(tri) and MR.euler(tri) == 2
    assert len(np.unique(tri["v"])) == len(vert)                  # all weights count: every vertex is used
    volume = MR.signed_volume(vert, tri)
    r = (min(dims) / 2 - 1.6) * v.voxel
    print(f"sphere {dims}, zeros below {zero_below}: {len(vert)} vertices, {len(tri)} triangles, volume {volume:.5f} (ball: {4.19 * r ** 3:.5f})")
    assert 0.5 * 4.19 * r ** 3 < volume < 1.5 * 4.19 * r ** 3     # positive: the normals point to free space
    assert np.all(np.diff(vert["id"].astype(np.int64)) > 0) and np.all(np.diff(tri["cell"].astype(np.int64)) >= 0)
    if zero_below:
        tq, _ = VR.unpack(vox)
        assert (tq == 0).sum() > 20
        p = np.stack([vert["x"], vert["y"], vert["z"]], axis=1)[tri["v"]]
        assert (np.all(p[:, 0] == p[:, 1], axis=1) | np.all(p[:, 1] == p[:, 2], axis=1)).any()          # coincident vertices are emitted


def test_random_signs_inside_a_positive_border_are_closed():
    v, vox = random_volume((10, 9, 8), 1, weights=False, border=True)
    vert, tri = MR.mesh(vox, v, 1)
    assert len(tri) > 1000 and MR.closed(tri)
    # without the border the surface runs out of the grid, and with weights some cells are not meshed: open, unreferenced vertices
    v, vox = random_volume((10, 9, 8), 2)
    vert, tri = MR.mesh(vox, v, 1)
    assert len(tri) > 100 and not MR.closed(tri) and len(np.unique(tri["v"])) < len(vert)
    assert len(MR.mesh(vox, v, 2)[1]) < len(tri) and len(MR.mesh(vox, v, 3)[0]) == 0


def test_the_generated_table_is_the_geometric_rule_and_the_one_in_the_source():
    gen = mesh_table()
    table = gen.table()
    seen = 0
    for t in range(6):
        for mask in range(16):
            assert table[t][mask] == MR.case_codes(t, mask), (t, mask)
            bits = bin(mask).count("1")
            assert len(MR.case_triangles(t, mask)) == (0 if bits in (0, 4) else 2 - bits % 2)            # what the kernels count by
            seen += bits not in (0, 4)
    assert seen == 84
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_mesh.hip")) as fh:
        body = re.search(r"MESH_TABLE\[6\]\[16\]\[2\] = \{\n(.*?)\n\};", fh.read(), re.S).group(1)
    assert body.split("\n") == gen.rows()
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "mesh_table.py")], capture_output=True, text=True, check=True)
    assert out.stdout.rstrip("\n").split("\n") == gen.rows()
    # every tetrahedron edge is one of the seven kinds from its lower corner, and the six tetrahedra use each face diagonal alike
    for t in range(6):
        p = MR.tet_corners(t)
        for a in range(4):
            for b in range(a + 1, 4):
                assert tuple(p[b] - p[a]) in MR.KINDS


@pytest.mark.parametrize("min_weight", [1, 2])
def test_axis_vertices_are_the_surface_points(min_weight):
    for v, vox in (MR.sphere((12, 11, 10)), random_volume((10, 9, 8), 3), random_volume((1, 9, 8), 4), random_volume((5, 1, 1), 5)):
        vert = MR.vertices(vox, v, min_weight)
        pts = VR.crossings(vox, v, min_weight)
        axis = vert[(vert["id"] & 7) < 3]
        assert len(pts) == len(axis)
        if min(v.nx, v.ny, v.nz) > 1 and len(pts):                # (the sphere's weights are 1: nothing at min_weight 2)
            assert len(axis) < len(vert)                          # the diagonals carry vertices too
        for name in "xyz":
            assert axis[name].tobytes() == pts[name].tobytes(), name
        assert np.array_equal((axis["id"] >> 3) * 4 + (axis["id"] & 7), pts["id"])


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

def c_volume(v):
    import soc_project_stereo_matching_amd as S
    return S.volume_spec(v.nx, v.ny, v.nz, v.voxel, v.origin, v.trunc, v.max_weight)


def test_header_library_and_python_agree():
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    lib = S.load_library()
    assert "sgm_volume_mesh" in _declared_functions() and hasattr(lib, "sgm_volume_mesh")
    for name in ("sgmd_volume_mesh", "sgmd_mesh_scratch_bytes"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    assert re.search(r"typedef struct \{ float x, y, z; uint32_t id; \} sgm_mesh_vertex;", text)
    assert re.search(r"typedef struct \{ uint32_t v\[3\]; uint32_t cell; \} sgm_mesh_triangle;", text)
    for line in ("nx*ny*nz <= 2^27", "(ac, ad, bd) then (ac, bd, bc)", "((v1-v0) x (v2-v0)) . (centroid(P) - centroid(N)) > 0"):
        assert line in text, line
    assert C.sizeof(S.SGMMeshVertex) == 16 and C.sizeof(S.SGMMeshTriangle) == 16
    assert [(n, getattr(S.SGMMeshVertex, n).offset) for n, _ in S.SGMMeshVertex._fields_] == [("x", 0), ("y", 4), ("z", 8), ("id", 12)]
    assert [(n, getattr(S.SGMMeshTriangle, n).offset) for n, _ in S.SGMMeshTriangle._fields_] == [("v", 0), ("cell", 12)]
    assert S.MESH_VERTEX_DTYPE == MR.VERTEX and S.MESH_TRIANGLE_DTYPE == MR.TRIANGLE and MR.VERTEX.itemsize == MR.TRIANGLE.itemsize == 16
    assert [MR.TRIANGLE.fields[n][1] for n in ("v", "cell")] == [0, 12]
    assert callable(getattr(S.SGMInstance, "volume_mesh", None))
    lib.sgmd_mesh_scratch_bytes.restype, lib.sgmd_mesh_scratch_bytes.argtypes = _z, [_i] * 3
    assert lib.sgmd_mesh_scratch_bytes(20, 17, 13) == 3 * 16 and lib.sgmd_mesh_scratch_bytes(0, 1, 1) == 0
    assert lib.sgmd_mesh_scratch_bytes(512, 512, 512) == 16 << 16


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

def _sign(L):
    for name, (res, args) in {"sgm_volume_mesh": (_b, [_p] * 3 + [_u, _p, _z, _p, _z, _p]),
                              "sgm_volume_points": (_b, [_p] * 3 + [_u, _p, _z, _p]),
                              "stub_mesh_clear": (None, []), "stub_mesh_count": (_i, []), "stub_mesh_ptr": (_p, [_i, _i]),
                              "stub_mesh_min_weight": (C.c_uint, [_i]), "stub_mesh_capacity": (_z, [_i, _i]),
                              "stub_mesh_fail_at": (None, [_i]), "stub_fail_alloc_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("meshstub"), extra_sources=[STUB_MESH, STUB_VOLUME], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    """the volume without the mesh"""
    return _sign(standin.build(tmp_path_factory.mktemp("meshstub_without"), extra_sources=[STUB_VOLUME], flags=("-ffp-contract=off",)))


class Buffers:
    """a caller's "device" buffers on the stand-in: host memory, the outputs pre-filled with 0xA5, 0xA5 words behind the volume"""
    def __init__(self, v, vox):
        self.n = v.nx * v.ny * v.nz
        self.voxels = np.full(self.n + 4, A5, np.uint32)
        self.voxels[:self.n] = np.asarray(vox, np.uint32).reshape(-1)
        self.before = self.voxels.copy()
        self.vertices = np.full(4 * (7 * self.n + 4), A5, np.uint32)
        self.triangles = np.full(4 * (12 * self.n + 4), A5, np.uint32)
        self.counts = np.full(4, A5, np.uint32)

    def poison(self):
        self.vertices[:] = A5
        self.triangles[:] = A5
        self.counts[:] = A5

    def untouched(self):
        return bool(np.all(self.vertices == A5) and np.all(self.triangles == A5) and np.all(self.counts == A5) and np.array_equal(self.voxels, self.before))

    def lists(self, nv, nt):
        """the first nv vertex and nt triangle records; everything behind them still 0xA5, the volume as it was"""
        assert np.all(self.vertices[4 * nv:] == A5) and np.all(self.triangles[4 * nt:] == A5) and np.all(self.counts[2:] == A5)
        assert np.array_equal(self.voxels, self.before)
        return self.vertices[:4 * nv].view(MR.VERTEX), self.triangles[:4 * nt].view(MR.TRIANGLE)


def mesh_call(L, s, cv, b, min_weight=1, vcap=None, tcap=None, voxels="own", vertices="own", triangles="own", counts="own"):
    pick = lambda given, own: own.ctypes.data if isinstance(given, str) else given
    return L.sgm_volume_mesh(s, None if cv is None else C.byref(cv), pick(voxels, b.voxels), min_weight, pick(vertices, b.vertices),
                             7 * b.n if vcap is None else vcap, pick(triangles, b.triangles), 12 * b.n if tcap is None else tcap,
                             pick(counts, b.counts))


def test_the_callers_pointers_arrive_and_the_scratch_is_reserved_reused_and_grown(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: the mesh needs no shape
    v, vox = MR.sphere((12, 11, 10))
    b = Buffers(v, vox)
    cv = c_volume(v)
    want = MR.mesh(vox, v, 1)
    L.stub_clear(); L.stub_mesh_clear()
    assert mesh_call(L, s, cv, b)
    assert L.stub_mesh_count() == 1 and L.stub_mesh_min_weight(0) == 1
    assert (L.stub_mesh_capacity(0, 0), L.stub_mesh_capacity(0, 1)) == (7 * b.n, 12 * b.n)
    assert [L.stub_mesh_ptr(0, k) for k in (0, 2, 3, 4)] == [b.voxels.ctypes.data, b.vertices.ctypes.data, b.triangles.ctypes.data, b.counts.ctypes.data]
    scratch = L.stub_mesh_ptr(0, 1)
    assert scratch is not None
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", 0)]                                          # 16 bytes, logged in KiB
    assert b.counts[:2].tolist() == [len(want[0]), len(want[1])]
    same_mesh("sphere", b.lists(*b.counts[:2]), want)
    # the scratch is kept: the same call again, and a smaller volume, allocate nothing
    L.stub_clear()
    b.poison()
    assert mesh_call(L, s, cv, b, min_weight=2) and b.counts[:2].tolist() == [0, 0] and b.lists(0, 0)
    v2, vox2 = random_volume((4, 3, 2), 7)
    b2 = Buffers(v2, vox2)
    assert mesh_call(L, s, c_volume(v2), b2)
    same_mesh("small", b2.lists(*b2.counts[:2]), MR.mesh(vox2, v2, 1))
    assert standin.launches(L, drop=()) == [] and L.stub_mesh_ptr(2, 1) == scratch
    # a larger one (three tiles of 2048 voxels, the last partial) grows it: a drain and an allocation of the new size
    v3, vox3 = MR.sphere((20, 17, 13))
    b3 = Buffers(v3, vox3)
    L.stub_clear()
    assert mesh_call(L, s, c_volume(v3), b3)
    assert standin.launches(L, drop=()) == [("sync", 0), ("alloc", 0)] and L.stub_mesh_ptr(3, 1) != scratch
    want3 = MR.mesh(vox3, v3, 1)
    same_mesh("three tiles", b3.lists(*b3.counts[:2]), want3)
    assert MR.closed(want3[1]) and MR.euler(want3[1]) == 2
    L.sgm_destroy(s)


@pytest.mark.parametrize("seed", [11, 12])
def test_the_stand_in_is_the_restatement_on_random_volumes(host, seed):
    L = host
    s = L.sgm_create(0)
    for dims in ((10, 9, 8), (1, 9, 8), (2, 2, 2), (5, 1, 1), (3, 2, 1)):
        v, vox = random_volume(dims, seed)
        b = Buffers(v, vox)
        for mw in (1, 2):
            b.poison()
            assert mesh_call(L, s, c_volume(v), b, min_weight=mw)
            same_mesh(f"{dims} min_weight {mw}", b.lists(*b.counts[:2]), MR.mesh(vox, v, mw))
    L.sgm_destroy(s)


def test_capacities_clip_the_lists_and_never_the_counts(host):
    L = host
    s = L.sgm_create(0)
    v, vox = MR.sphere((9, 13, 7))
    cv = c_volume(v)
    b = Buffers(v, vox)
    vert, tri = MR.mesh(vox, v, 1)
    nv, nt = len(vert), len(tri)
    for vcap, tcap, wv, wt in ((0, 0, 0, 0), (nv, nt, nv, nt), (nv - 1, nt, nv - 1, 0), (nv, nt - 1, nv, nt - 1), (nv + 3, nt + 3, nv, nt),
                               (nv, 0, nv, 0), (0, nt, 0, 0)):
        b.poison()
        none = dict(vertices=None) if vcap == 0 else {}
        if tcap == 0:
            none["triangles"] = None
        assert mesh_call(L, s, cv, b, vcap=vcap, tcap=tcap, **none), (vcap, tcap)
        assert b.counts[:2].tolist() == [nv, nt], (vcap, tcap)
        same_mesh(f"capacities {vcap} {tcap}", b.lists(wv, wt), (vert[:wv], tri[:wt]))
    L.sgm_destroy(s)


NAN, INF = float("nan"), float("inf")
SPEC_REFUSALS = {
    "nx 0": dict(nx=0), "nx 1025": dict(nx=1025), "ny -1": dict(ny=-1), "nz 1025": dict(nz=1025), "voxel 0": dict(voxel=0.0),
    "voxel NaN": dict(voxel=NAN), "origin INF": dict(origin=(INF, 0, 0)), "trunc NaN": dict(trunc=NAN), "max_weight 0": dict(max_weight=0),
    "max_weight 65536": dict(max_weight=65536),
    "2^27 + 2^20 voxels": dict(nx=1024, ny=1024, nz=129), "2^30 voxels": dict(nx=1024, ny=1024, nz=1024),
}


def test_every_refusal_queues_nothing(host, capfd):
    L = host
    s = L.sgm_create(0)
    v, vox = MR.sphere((9, 13, 7))
    cv = c_volume(v)
    b = Buffers(v, vox)
    x, q, t, k = b.voxels.ctypes.data, b.vertices.ctypes.data, b.triangles.ctypes.data, b.counts.ctypes.data
    mc = lambda **kw: mesh_call(L, s, cv, b, **kw)
    L.stub_clear(); L.stub_mesh_clear()
    capfd.readouterr()
    refusals = [
        lambda: mesh_call(L, None, cv, b), lambda: mesh_call(L, s, None, b), lambda: mc(voxels=None), lambda: mc(counts=None),
        lambda: mc(vertices=None), lambda: mc(triangles=None), lambda: mc(vertices=None, vcap=1, tcap=0, triangles=None),
        lambda: mc(min_weight=0), lambda: mc(min_weight=65536),
        lambda: mc(voxels=x + 2), lambda: mc(vertices=q + 8), lambda: mc(vertices=q + 4), lambda: mc(triangles=t + 8), lambda: mc(counts=k + 2),
        # outputs that overlap the volume or each other, from the first to the last byte
        lambda: mc(vertices=x + (-x % 16)), lambda: mc(triangles=x + (-x % 16)), lambda: mc(counts=x), lambda: mc(counts=x + 4 * (b.n - 1)),
        lambda: mc(triangles=q), lambda: mc(triangles=q + 16 * (7 * b.n - 1)), lambda: mc(counts=q + 16), lambda: mc(counts=t + 16 * 12 * b.n - 4),
        lambda: mc(counts=q - 4, vcap=1),
    ]
    for name, kw in SPEC_REFUSALS.items():
        d = dict(nx=9, ny=13, nz=7, voxel=0.05, origin=(0, 0, 0), trunc=0.1, max_weight=4)
        d.update(kw)
        refusals.append(lambda d=d: mesh_call(L, s, c_volume(VR.spec(**d)), b))
    for n, call in enumerate(refusals):
        assert not call(), n
        err = capfd.readouterr().err
        assert err.startswith("sgm_mi355x: sgm_volume_mesh: ") and err.count("\n") == 1, (n, err)
    assert L.stub_mesh_count() == 0 and standin.log(L) == [] and b.untouched()
    # allowed: 2^27 voxels exactly (the stand-in only logs so large a volume), the counts right behind the records asked for,
    # counts alone without arrays
    big = VR.spec(1024, 1024, 128, 0.01, (0, 0, 0), 0.1)
    assert mesh_call(L, s, c_volume(big), b, vcap=0, tcap=0, vertices=None, triangles=None) and L.stub_mesh_count() == 1
    assert mc(vcap=2, tcap=0, triangles=None, counts=q + 32)
    assert mc(vcap=0, tcap=0, vertices=None, triangles=None) and b.counts[0] > 0
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_refuses_and_keeps_the_volume(host_without, capfd):
    L = host_without
    s = L.sgm_create(0)
    v, vox = MR.sphere((9, 13, 7))
    b = Buffers(v, vox)
    capfd.readouterr()
    L.stub_clear()
    assert not mesh_call(L, s, c_volume(v), b)
    assert "sgm_mi355x: sgm_volume_mesh: the mesh is not part of this build" in capfd.readouterr().err
    assert standin.log(L) == [] and b.untouched()
    assert L.sgm_volume_points(s, C.byref(c_volume(v)), b.voxels.ctypes.data, 1, None, 0, b.counts.ctypes.data) and b.counts[0] > 0
    L.sgm_destroy(s)


def test_an_instance_that_never_meshes_is_the_instance_it_was(host, host_without):
    import soc_project_stereo_matching_amd as S
    w, h = 48, 20
    left, right = np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)
    out = np.zeros((h, w), np.float32)
    logs = []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        assert L.sgm_reset(s, w, h, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        L.sgm_destroy(s)
    assert logs[0] == logs[1] and len(logs[0]) > 10


def test_a_refused_launch_allocation_or_wait_fails_the_call_and_leaves_the_outputs(host):
    import soc_project_stereo_matching_amd as S
    L = host
    w, h = 48, 20
    s = L.sgm_create(0)
    opt = S.default_option(16)
    assert L.sgm_reset(s, w, h, C.byref(opt))
    v, vox = MR.sphere((9, 13, 7))
    cv = c_volume(v)
    b = Buffers(v, vox)
    # the first allocation of the scratch, refused
    L.stub_mesh_clear()
    L.stub_fail_alloc_at(0)
    ok = mesh_call(L, s, cv, b)
    L.stub_fail_alloc_at(-1)
    assert not ok and b.untouched() and L.stub_mesh_count() == 0
    # a launch, refused: reported, the outputs untouched, and the instance goes on
    L.stub_mesh_fail_at(0)
    assert not mesh_call(L, s, cv, b) and b.untouched()
    assert mesh_call(L, s, cv, b) and b.counts[1] == len(MR.mesh(vox, v, 1)[1]) > 0
    # with the post pass on a stream of its own the call waits for the result of a match that is still in flight
    left = np.zeros((h, w), np.uint8)
    out = np.zeros((h, w), np.float32)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, w, h, C.byref(opt))
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    L.stub_clear()
    assert mesh_call(L, s, cv, b) and "wait_event" in [e.name for e in standin.log(L)]
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, out.ctypes.data)
    L.stub_clear()
    L.stub_fail_at(b"wait_event", 0)
    L.stub_mesh_clear()
    assert not mesh_call(L, s, cv, b) and L.stub_mesh_count() == 0
    assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_mesh_host_is_asan_ubsan_clean(tmp_path):
    """tests/mesh_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in mesh."""
    exe = standin.build(tmp_path, sanitize=True, exe="mesh_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "mesh_sanitize_driver.c"), STUB_MESH, STUB_VOLUME])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("mesh_sanitize_driver ok")
