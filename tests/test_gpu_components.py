"""Connected components of the TSDF volume on the device (extension; include/sgm_mi355x.h, the components section) against the numpy
restatement tests/components_ref.py -- needs an MI355X.  Tolerance 0 everywhere: words and bytes are compared.  Every array a call
may write sits between margins of 0xA5 and is pre-filled (with 0xA5 unless the test says otherwise), the margins are checked
afterwards and the volume compared unchanged.  The cases are those of tests/components_cases.py, which tests/test_zz_components_cpu.py
holds against an independent flood fill on the restatement alone."""
import numpy as np
import pytest

import components_cases as CC
import components_ref as CR
import mesh_ref as MR
import volume_ref as VR
from test_distance_cpu import fused_scene
from test_gpu_raycast import Between
from test_gpu_volume import c_source, c_volume, upload
from test_gpu_volume_distance import Off

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

REC = CR.COMPONENT.itemsize


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: the components need no shape
    yield i
    i.close()


def plane_records(planes):
    import soc_project_stereo_matching_amd as S
    out = np.zeros(len(planes), S.PLANE_DTYPE)
    for q, (normal, anchor) in enumerate(planes):
        out[q]["normal"], out[q]["anchor"] = normal, anchor
        out[q]["offset"] = -np.dot(np.asarray(normal, np.float64), np.asarray(anchor, np.float64))
    return out


def device_components(inst, v, words, label, min_weight=1, set=0, unknown=0, connectivity=6, min_voxels=1, planes=(), clearance=(),
                      capacity=None, d_vox=None, fill=0xA5):
    """one call: (labels uint32 [nz][ny][nx], the bytes of the object array, counts [2]); capacity None: room for every voxel's own
    component; d_vox: the volume on the device, made here (and checked as only read) unless given"""
    import torch
    import soc_project_stereo_matching_amd as S
    own = d_vox is None
    if own:
        d_vox = Off(words.nbytes, words)
    capacity = words.size if capacity is None else capacity
    d_lab = Off(4 * words.size, fill=fill)
    d_obj = Between(max(REC * capacity, 16))
    d_cnt = Between(8)
    comp = S.component_spec(min_weight, set, unknown, connectivity, min_voxels, plane_records(planes), clearance)
    torch.cuda.synchronize()
    assert inst.volume_components(c_volume(v), comp, d_vox.ptr, d_lab.ptr, d_obj.ptr if capacity else None, capacity, d_cnt.ptr), label
    assert inst.synchronize(), label
    labels = d_lab.read(label + " labels", np.uint32).reshape(words.shape).copy()
    objects = d_obj.read(label + " objects").copy()
    counts = d_cnt.read(label + " counts", np.uint32).copy()
    if own:
        assert d_vox.read(label + " volume").tobytes() == np.ascontiguousarray(words).tobytes(), f"{label}: the volume is only read"
    return labels, objects, counts


def same_result(label, got, want, capacity):
    """labels word for word, both counts, the records that exist byte for byte and nothing written behind them"""
    labels, raw, counts = got
    want_labels, want_objects, want_counts = want
    if not np.array_equal(labels, want_labels):
        bad = np.argwhere(labels != want_labels)
        k, j, i = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {labels.size} labels differ, first at (i, j, k) = ({i}, {j}, {k}): "
                             f"{int(labels[k, j, i])} for {int(want_labels[k, j, i])}")
    assert tuple(counts) == tuple(want_counts), (label, tuple(counts), want_counts)
    written = min(want_counts[0], capacity)
    got_objects = raw[:REC * written].view(CR.COMPONENT)
    assert got_objects.tobytes() == want_objects[:written].tobytes(), (label, got_objects[:4], want_objects[:4])
    assert np.all(raw[REC * written:] == 0xA5), f"{label}: wrote behind the {written} records that exist"


def check(inst, v, words, label, capacity=None, **kw):
    capacity = words.size if capacity is None else capacity
    ref = {k: kw[k] for k in ("min_weight", "set", "unknown", "connectivity", "min_voxels", "planes", "clearance") if k in kw}
    want = CR.call(words, v, ref.pop("min_weight", 1), **ref)
    got = device_components(inst, v, words, label, capacity=capacity, **kw)
    same_result(label, got, want, capacity)
    return got, want


# ---- 1. shapes and options -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", CC.SMALL_DIMS)
def test_small_volumes_at_every_density_connectivity_and_set(inst, dims):
    calls = 0
    v = CC.spec_of(dims)
    for density, min_weight, words in CC.small_cases(dims):
        d_vox = Off(words.nbytes, words)
        for connectivity, set_, unknown in CC.OPTIONS:
            check(inst, v, words, f"{dims} density {density} min_weight {min_weight} conn {connectivity} set {set_} unknown {unknown}",
                  min_weight=min_weight, set=set_, unknown=unknown, connectivity=connectivity, d_vox=d_vox)
            calls += 1
        assert d_vox.read("volume").tobytes() == words.tobytes()
    assert calls == len(CC.DENSITIES) * 8


@pytest.mark.parametrize("dims", [(1, 1, 1), (CC.TX + 1, CC.TY + 1, CC.TZ + 1)])
def test_the_empty_set_the_full_set_and_a_checkerboard(inst, dims):
    v, n = CC.spec_of(dims), dims[0] * dims[1] * dims[2]
    for connectivity in (6, 26):
        (labels, raw, counts), _ = check(inst, v, np.full((dims[2], dims[1], dims[0]), CC.OUT, np.uint32), f"{dims} empty", connectivity=connectivity)
        assert tuple(counts) == (0, 0) and not labels.any() and np.all(raw == 0xA5)
        (labels, raw, counts), _ = check(inst, v, np.full((dims[2], dims[1], dims[0]), CC.IN, np.uint32), f"{dims} full", connectivity=connectivity)
        obj = raw[:REC].view(CR.COMPONENT)[0]
        assert tuple(counts) == (1, 1) and np.all(labels == 1) and obj["voxels"] == n
        assert tuple(obj["lo"]) == (0, 0, 0) and tuple(obj["hi"]) == tuple(d - 1 for d in dims)
        (labels, raw, counts), _ = check(inst, v, CC.checkerboard(dims), f"{dims} checkerboard", connectivity=connectivity)
        assert tuple(counts) == ((((n + 1) // 2),) * 2 if connectivity == 6 else (1, 1))


# ---- 2. across tile borders ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_u_across_a_tile_face_is_one_component(inst, axis):
    dims, words = CC.u_across_a_face(axis)
    for connectivity in (6, 26):
        (labels, _, counts), _ = check(inst, CC.spec_of(dims), words, f"U along axis {axis} conn {connectivity}", connectivity=connectivity)
        assert tuple(counts) == (1, 1) and set(np.unique(labels)) == {0, int(labels.max())}


def test_a_comb_crossing_one_face_many_times(inst):
    dims, words = CC.comb()
    (_, _, counts), _ = check(inst, CC.spec_of(dims), words, "comb, 6", connectivity=6)
    assert tuple(counts) == (2, 2)
    (_, _, counts), _ = check(inst, CC.spec_of(dims), words, "comb, 26", connectivity=26)
    assert tuple(counts) == (1, 1)


def test_a_serpentine_through_three_tiles_in_each_axis(inst):
    """the expected result in closed form: one component of every voxel of the path, first 0"""
    dims, words, n = CC.serpentine()
    inside = words == CC.IN
    for connectivity in (6, 26):
        labels, raw, counts = device_components(inst, CC.spec_of(dims), words, f"serpentine {connectivity}", connectivity=connectivity, capacity=2)
        assert tuple(counts) == (1, 1)
        assert np.array_equal(labels, inside.astype(np.uint32))
        obj = raw[:REC].view(CR.COMPONENT)[0]
        k, j, i = np.nonzero(inside)
        assert obj["first"] == 0 and obj["voxels"] == n and tuple(obj["lo"]) == (0, 0, 0) and tuple(obj["hi"]) == (i.max(), j.max(), k.max())
        assert tuple(int(s) for s in obj["sum"]) == (int(i.sum()), int(j.sum()), int(k.sum())) and np.all(raw[REC:] == 0xA5)


def test_a_component_whose_smallest_voxel_lies_in_the_last_tile(inst):
    dims, words = CC.last_tile_only()
    (labels, raw, counts), _ = check(inst, CC.spec_of(dims), words, "last tile")
    first = int(raw[:REC].view(CR.COMPONENT)[0]["first"])
    i, j, k = first % dims[0], first // dims[0] % dims[1], first // (dims[0] * dims[1])
    assert tuple(counts) == (1, 1) and i >= CC.TX and j >= CC.TY and k >= CC.TZ


# ---- 3. the contract -----------------------------------------------------------------------------------------------------------

def test_min_voxels_at_below_and_above_a_components_size(inst):
    dims, words, sizes = CC.blobs()
    v = CC.spec_of(dims)
    for min_voxels in (1, 4, 5, 6, 7, 8, 12, 13):
        (labels, _, counts), (_, want_objects, _) = check(inst, v, words, f"min_voxels {min_voxels}", min_voxels=min_voxels)
        assert tuple(counts) == (sum(s >= min_voxels for s in sizes), len(sizes))
        assert [int(o["voxels"]) for o in want_objects] == [s for s in sizes if s >= min_voxels]
        assert (labels != 0).sum() == sum(s for s in sizes if s >= min_voxels)


def test_capacities_around_the_number_of_components(inst):
    dims, words, sizes = CC.blobs()
    v, C = CC.spec_of(dims), len(sizes)
    for capacity in (0, C - 1, C, C + 1):
        (_, _, counts), _ = check(inst, v, words, f"capacity {capacity}", capacity=capacity)
        assert tuple(counts) == (C, C)
    rng_words = CC.random_words(np.random.default_rng(7), (CC.TX + 1, CC.TY + 1, CC.TZ + 1), 0.3)
    want = CR.call(rng_words, CC.spec_of((CC.TX + 1, CC.TY + 1, CC.TZ + 1)), 1, min_voxels=2)
    for capacity in (0, want[2][0] - 1, want[2][0], want[2][0] + 1):
        check(inst, CC.spec_of((CC.TX + 1, CC.TY + 1, CC.TZ + 1)), rng_words, f"random, capacity {capacity}", capacity=capacity, min_voxels=2)


def test_plane_exclusion_takes_the_floor_out(inst):
    v, words, plane, clearance = CC.floor_and_boxes()
    (_, _, counts), _ = check(inst, v, words, "with the floor")
    assert tuple(counts) == (1, 1)
    (labels, _, counts), _ = check(inst, v, words, "floor excluded", planes=[plane], clearance=[clearance])
    assert tuple(counts) == (2, 2)
    assert not labels[:, 0:3, :].any() and labels[2, 3, 4] != 0    # layer 2 has s == clearance exactly: excluded; layer 3 stays
    # a smaller clearance leaves layer 2 in, and the boxes are one again through it
    (_, _, counts), _ = check(inst, v, words, "clearance below the layer", planes=[plane], clearance=[0.2])
    assert tuple(counts) == (1, 1)
    void = (np.array([0.0, -0.0, 0.0], np.float32), plane[1])
    (_, _, counts), _ = check(inst, v, words, "a void plane", planes=[void], clearance=[100.0])
    assert tuple(counts) == (1, 1)
    walls = [plane, void, ((1.0, 0.0, 0.0), (0.9, 0.0, 0.0)), ((0.0, 0.0, -1.0), (0.0, 0.0, 1.3))]
    check(inst, v, words, "four planes", planes=walls, clearance=[clearance, 1.0, 0.05, -0.1])
    check(inst, v, words, "four planes, free set", planes=walls, clearance=[clearance, 1.0, 0.05, -0.1], set=1, connectivity=26)


def test_two_calls_and_any_prefill_give_the_same_bytes(inst):
    dims = (2 * CC.TX + 5, CC.TY + 3, 2 * CC.TZ + 1)
    v, words = CC.spec_of(dims), CC.random_words(np.random.default_rng(99), dims, 0.35)
    kw = dict(connectivity=26, min_voxels=3, capacity=500)
    (first, raw, counts), _ = check(inst, v, words, "first", **kw)
    for fill in (0xA5, 0x00, 0xFF):
        labels, raw2, counts2 = device_components(inst, v, words, f"fill {fill:#x}", fill=fill, **kw)
        assert labels.tobytes() == first.tobytes() and raw2.tobytes() == raw.tobytes() and counts2.tobytes() == counts.tobytes()


# ---- 4. the objects of a list --------------------------------------------------------------------------------------------------

def device_component_of(inst, v, d_lab, d_obj, capacity, d_cnt, d_rec, rec_capacity, d_rec_count, id_kinds, label):
    import torch
    out = Between(4 * rec_capacity)
    torch.cuda.synchronize()
    assert inst.volume_component_of(c_volume(v), d_lab.ptr, d_obj.ptr, capacity, d_cnt.ptr, d_rec.ptr, rec_capacity,
                                    d_rec_count.ptr if d_rec_count is not None else None, id_kinds, out.ptr) and inst.synchronize(), label
    return out.read(label, np.uint32).copy()


def test_component_of_behind_the_mesh_and_the_points_of_a_fused_scene(inst):
    import torch
    import soc_project_stereo_matching_amd as S
    v, s, poses, disp, words0, fused = fused_scene()
    n = fused.size
    d_vox = Between(fused.nbytes, fused)
    want_labels, want_objects, (C, _) = CR.call(fused, v, 1, min_voxels=2)
    assert C >= 2
    vert, tri = MR.mesh(fused, v, 1)
    points = VR.crossings(fused, v, 1)
    # a record whose voxel n is the free end: its label comes from the other end of its edge
    assert np.any(want_labels.reshape(-1)[vert["id"] >> 3] == 0) and np.any(want_labels.reshape(-1)[points["id"] >> 2] == 0)
    for capacity in (C, C - 1):
        d_lab, d_obj, d_cnt = Between(4 * n), Between(REC * capacity), Between(8)
        d_vert, d_tri, d_mc = Between(16 * len(vert)), Between(16 * len(tri)), Between(8)
        d_pts, d_pc = Between(16 * len(points) + 16 * 5), Between(4)
        torch.cuda.synchronize()
        # queued back to back, the count words stay on the device
        assert inst.volume_mesh(c_volume(v), d_vox.ptr, 1, d_vert.ptr, len(vert), d_tri.ptr, len(tri), d_mc.ptr)
        assert inst.volume_points(c_volume(v), d_vox.ptr, 1, d_pts.ptr, len(points) + 5, d_pc.ptr)
        assert inst.volume_components(c_volume(v), S.component_spec(1, min_voxels=2), d_vox.ptr, d_lab.ptr, d_obj.ptr, capacity, d_cnt.ptr)
        idx_mesh = Between(4 * len(vert))
        idx_pts = Between(4 * (len(points) + 5))
        assert inst.volume_component_of(c_volume(v), d_lab.ptr, d_obj.ptr, capacity, d_cnt.ptr, d_vert.ptr, len(vert), d_mc.ptr, 8, idx_mesh.ptr)
        assert inst.volume_component_of(c_volume(v), d_lab.ptr, d_obj.ptr, capacity, d_cnt.ptr, d_pts.ptr, len(points) + 5, d_pc.ptr, 4, idx_pts.ptr)
        assert inst.synchronize()
        assert d_vert.read("vertices").tobytes() == vert.tobytes() and d_lab.read("labels", np.uint32).tobytes() == want_labels.tobytes()
        got = idx_mesh.read("mesh index", np.uint32)
        want = CR.component_of(want_labels, want_objects, capacity, vert["id"], 8)
        assert np.array_equal(got, want) and want.max() == capacity and (capacity == C or np.any((want == 0) & (CR.component_of(want_labels, want_objects, C, vert["id"], 8) != 0)))
        got = idx_pts.read("point index", np.uint32)
        want = CR.component_of(want_labels, want_objects, capacity, points["id"], 4)
        assert np.array_equal(got[:len(points)], want) and np.all(got[len(points):] == 0xA5A5A5A5)     # behind the count: not written
    assert d_vox.read("fused, afterwards").tobytes() == fused.tobytes()
    # without a count word every record of the capacity is handled; ids outside the volume or of no kind give 0
    ids = np.array([0, 8 * n, 8 * n - 1, 7, 0xFFFFFFFF, vert["id"][0]], np.uint32)
    rec = np.zeros(len(ids), MR.VERTEX)
    rec["id"] = ids
    d_lab, d_obj, d_cnt = Between(4 * n, want_labels), Between(REC * C, want_objects), Between(8, np.array([C, C], np.uint32))
    got = device_component_of(inst, v, d_lab, d_obj, C, d_cnt, Between(rec.nbytes, rec), len(ids), None, 8, "loose ids")
    assert np.array_equal(got, CR.component_of(want_labels, want_objects, C, ids, 8))


# ---- 5. refusals on the device build -------------------------------------------------------------------------------------------

def test_refusals_leave_the_poisoned_outputs_untouched(inst, capfd):
    import soc_project_stereo_matching_amd as S
    dims = (12, 6, 5)
    v, words = CC.spec_of(dims), CC.random_words(np.random.default_rng(3), dims, 0.2)
    n = words.size
    d_vox, d_lab, d_obj, d_cnt, d_rec, d_idx = Between(4 * n, words), Between(4 * n), Between(REC * 8), Between(8), Between(16 * 4), Between(16)
    ok, cv = S.component_spec(1), c_volume(v)
    bad_volume = c_volume(VR.spec(0, 6, 5, 0.0625, (0, 0, 0), 0.25))
    nan_plane = plane_records([((0.0, np.nan, 0.0), (0.0, 0.0, 0.0))])
    fine_plane = plane_records([((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))])
    comp = lambda c, **kw: inst.volume_components(kw.get("v", cv), c, kw.get("vox", d_vox.ptr), kw.get("lab", d_lab.ptr),
                                                  kw.get("obj", d_obj.ptr), kw.get("cap", 8), kw.get("cnt", d_cnt.ptr))
    of = lambda **kw: inst.volume_component_of(kw.get("v", cv), kw.get("lab", d_lab.ptr), kw.get("obj", d_obj.ptr), 8, kw.get("cnt", d_cnt.ptr),
                                               kw.get("rec", d_rec.ptr), 4, kw.get("rc", None), kw.get("kinds", 8), kw.get("idx", d_idx.ptr))
    refusals = [
        lambda: comp(ok, v=bad_volume), lambda: comp(ok, vox=None), lambda: comp(ok, lab=None), lambda: comp(ok, cnt=None),
        lambda: comp(ok, obj=None), lambda: comp(S.component_spec(0)), lambda: comp(S.component_spec(65536)),
        lambda: comp(S.component_spec(1, set=2)), lambda: comp(S.component_spec(1, unknown=-1)), lambda: comp(S.component_spec(1, connectivity=18)),
        lambda: comp(S.component_spec(1, min_voxels=0)), lambda: comp(S.component_spec(1, planes=np.zeros(5, S.PLANE_DTYPE), clearance=[0] * 5)),
        lambda: comp(S.component_spec(1, planes=nan_plane, clearance=[0.0])), lambda: comp(S.component_spec(1, planes=fine_plane, clearance=[np.inf])),
        lambda: comp(ok, vox=d_vox.ptr + 2), lambda: comp(ok, lab=d_lab.ptr + 1), lambda: comp(ok, obj=d_obj.ptr + 4), lambda: comp(ok, cnt=d_cnt.ptr + 2),
        lambda: comp(ok, lab=d_vox.ptr + 4 * n - 4), lambda: comp(ok, cnt=d_lab.ptr), lambda: comp(ok, obj=d_lab.ptr + 8),
        lambda: of(v=bad_volume), lambda: of(lab=None), lambda: of(cnt=None), lambda: of(rec=None), lambda: of(idx=None), lambda: of(kinds=6),
        lambda: of(rec=d_rec.ptr + 8), lambda: of(obj=d_obj.ptr + 4), lambda: of(idx=d_idx.ptr + 2), lambda: of(rc=d_cnt.ptr + 1),
        lambda: of(idx=d_rec.ptr), lambda: of(idx=d_lab.ptr + 16),
    ]
    for k, call in enumerate(refusals):
        capfd.readouterr()
        assert not call(), k
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("sgm_mi355x: sgm_volume_component"), (k, err)
    assert inst.synchronize()
    for name, b in (("labels", d_lab), ("objects", d_obj), ("counts", d_cnt), ("index", d_idx)):
        assert np.all(b.read(name) == 0xA5), name
    assert d_vox.read("volume").tobytes() == words.tobytes()
