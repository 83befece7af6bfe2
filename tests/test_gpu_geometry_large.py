"""The geometry kernels beyond one lap, one scan chunk and one tile's distance, and at the ends of the admitted image sizes -- needs an
MI355X.  The cases are those of tests/geometry_large.py:

  track    frames of more lane items than TRACK_MAX_BLOCKS workgroups hold, on both load paths: sgm_track_sums_k goes round its
           stride loop again; sums past 2^53, and the host's reading of them into its solve;
  cloud    batches of more than SCAN_THREADS * SCAN_PER_THREAD tiles: tile_scan carries into a second chunk, and a frame's offsets
           word is written from it; frames 65535 wide or tall;
  volume   a volume of 4128 tiles: the scans of sgm_volume_points and sgm_volume_mesh (twice) carry, and mesh_cell_vertices finds
           the records of corner voxels 24 tiles up, across the chunk; a layer of two tiles; all 64 pose slots of the integration;
  slivers  ray-cast views, tracked model maps, registration targets and sources 65535 wide or tall.

Tolerance 0 everywhere, against the numpy restatements: outputs between (or in front of) margins of 0xA5 that are checked afterwards,
inputs checked as only read -- by the helpers of the six GPU files, which these tests reuse.  test_geometry_large_cpu.py asserts on
the restatements alone that every case reaches what it is for.  NOTES.md has the shapes, the counts and the wall times."""
import numpy as np
import pytest

import cloud_ref as CR
import geometry_large as GL
import test_gpu_cloud as GC
import test_gpu_mesh as GM
import test_gpu_raycast as GRC
import test_gpu_register as GG
import test_gpu_volume as GV
import track_ref as TR
import volume_ref as VR
from test_gpu_track import Inputs, device_sums
from test_mesh_cpu import random_volume, same_mesh
from test_raycast_cpu import same_maps
from test_track_cpu import c_model

# (the cached cases are read-only on purpose; torch remarks on that where a helper wraps one to copy it to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: explicit maps need no shape
    yield i
    i.close()


# ---- track ---------------------------------------------------------------------------------------------------------------------

def track_inputs(name, sides, skew=False):
    s, disp, m, poses, depth, normal, mask, conf = GL.track_case(name)
    return s, m, poses, Inputs(disp, depth, normal, mask if sides else None, conf if sides else None, skew)


@pytest.mark.parametrize("name", list(GL.TRACK_SHAPES))
def test_track_frames_beyond_one_lap_of_the_grid(inst, name):
    for sides in (True, False):
        s, m, poses, inp = track_inputs(name, sides)
        got = device_sums(inst, s, m, poses, inp, f"{name} side maps={sides}")
        assert got.tolist() == GL.track_want(name, sides).tolist(), (name, sides)


def test_track_maps_one_element_off_take_five_laps_of_one_pixel(inst):
    name = GL.TRACK_SKEWED
    for sides in (True, False):
        s, m, poses, inp = track_inputs(name, sides)
        aligned = device_sums(inst, s, m, poses, inp, f"{name} aligned")
        s, m, poses, inp = track_inputs(name, sides, skew=True)
        skewed = device_sums(inst, s, m, poses, inp, f"{name} skewed")
        assert skewed.tobytes() == aligned.tobytes() and skewed.tolist() == GL.track_want(name, sides).tolist(), sides


def test_track_a_batch_equals_frame_by_frame_and_runs_repeat_beyond_one_lap(inst):
    name = GL.TRACK_SKEWED
    s, disp, m, poses, depth, normal, mask, conf = GL.track_case(name)
    inp = Inputs(disp, depth, normal, mask, conf)
    runs = [device_sums(inst, s, m, poses, inp, "batch") for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes() and runs[0].tolist() == GL.track_want(name, True).tolist()
    one = type(s)(**dict(vars(s), frames=1))
    for f in range(s.frames):
        got = device_sums(inst, one, m, poses[f:f + 1], Inputs(disp[f], depth[f], normal[f], mask[f], conf[f]), f"frame {f}")
        assert got[0].tobytes() == runs[0][f].tobytes(), f


def test_track_sums_past_53_bits_and_the_hosts_reading_of_them(inst):
    s, disp, m, poses, depth, normal = GL.track_big()
    inp = Inputs(disp, depth, normal)
    got = device_sums(inst, s, m, poses, inp, "four laps")
    want = GL.track_big_want()
    assert got.tolist() == want.tolist()
    # one round of sgm_track on the same maps: the host reads these sums into doubles in the contract's order
    guess = np.asarray(poses, np.float64)
    out = inst.track(GV.c_source(s), c_model(m), guess, inp.ptr("disp"), None, None, inp.ptr("depth"), inp.ptr("normal"), trace=True)
    assert out is not None
    got_poses, got_stats, t_sums, t_poses = out
    inp.only_read("track")
    w_poses, w_stats, w_sums, w_trace = TR.track(disp, s, m, guess, depth, normal)
    assert t_sums.tobytes() == w_sums.tobytes() and w_sums[0].tolist() == want.tolist()
    assert got_poses.tobytes() == w_poses.tobytes() and got_stats == w_stats and t_poses.tobytes() == w_trace.tobytes()
    assert w_stats[0]["status"] == 0 and w_poses.tobytes() != guess.tobytes()


# ---- cloud ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", GL.CLOUD_VARIANTS)
@pytest.mark.parametrize("name", list(GL.CLOUD_BATCHES))
def test_cloud_batches_of_more_tiles_than_one_chunk_of_the_scan(inst, name, variant):
    """all frames + 1 offsets, every record, the organised cloud and what stays unwritten: test_gpu_cloud.check"""
    s, disp, mask, conf, keep = GL.cloud_batch(name, variant)
    label = f"{name} {s.width}x{s.height}x{s.frames} {variant}"
    assert GC.check(inst, s, disp, mask, conf, label) == keep.sum()
    if name == "one partial tile a frame":                        # ... and one float off an aligned allocation
        assert GC.check(inst, s, disp, mask, conf, label + " misaligned", misalign=True) == keep.sum()


@pytest.mark.parametrize("size", GL.CLOUD_SLIVERS, ids=GL.sliver_name)
def test_cloud_frames_65535_wide_or_tall(inst, size):
    s, disp, mask, conf, keep = GL.cloud_sliver(*size)
    assert GC.check(inst, s, disp, mask, conf, f"cloud {size}") == keep.sum()
    assert GC.check(inst, s, disp, None, None, f"cloud {size} misaligned, no side maps", misalign=True) == CR.kept(disp, s)[0].sum()


# ---- volume --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """the big volume on the device, once: (spec, words, test_gpu_mesh.Device, test_gpu_volume.Device)"""
    v, words = GL.big_volume()
    return v, words, GM.Device(v, words), GV.Device(v, words)


def big_points_once(inst, big, min_weight, capacity, label):
    v, words, _, vdev = big
    got = vdev.extract(inst, min_weight, capacity, label)
    assert vdev.words(label).tobytes() == words.tobytes(), f"{label}: the volume is only read"
    return got


@pytest.mark.parametrize("min_weight", GL.MIN_WEIGHTS)
def test_big_volume_surface_points(inst, big, min_weight):
    want = GL.big_points(min_weight)
    label = f"{GL.BIG_DIMS} points, min_weight {min_weight}"
    GV.same_list(label, big_points_once(inst, big, min_weight, len(want) + 2, label), want)


@pytest.mark.parametrize("min_weight", GL.MIN_WEIGHTS)
def test_big_volume_mesh(inst, big, min_weight):
    want = GL.big_mesh(min_weight)
    label = f"{GL.BIG_DIMS} mesh, min_weight {min_weight}"
    nv, nt, vert, tri = big[2].mesh(inst, min_weight, len(want[0]) + 2, len(want[1]) + 2, label)
    assert (nv, nt) == (len(want[0]), len(want[1])), label
    same_mesh(label, (vert, tri), want)


def test_big_volume_with_capacities_one_short(inst, big):
    """the counts stay full and the lists are clipped (Device.mesh and Device.extract check what stays 0xA5)"""
    pts = GL.big_points(1)
    got = big_points_once(inst, big, 1, len(pts) - 1, "points one short")
    assert len(got[1]) == len(pts) - 1
    GV.same_list("points one short", got, pts)
    want_v, want_t = GL.big_mesh(1)
    full = (len(want_v), len(want_t))
    for vcap, tcap in ((full[0] - 1, full[1]), (full[0], full[1] - 1)):
        label = f"mesh capacities {vcap} {tcap}"
        nv, nt, vert, tri = big[2].mesh(inst, 1, vcap, tcap, label)
        assert (nv, nt) == full, label
        assert len(vert) == vcap and len(tri) == (tcap if vcap == full[0] else 0), label          # a clipped vertex list: no triangle
        same_mesh(label, (vert, tri), (want_v[:len(vert)], want_t[:len(tri)]))


@pytest.mark.parametrize("kind", ["sphere", "random"])
def test_mesh_of_a_layer_of_two_tiles(inst, kind):
    v, words = GL.two_tile_layer(kind)
    for mw in GL.MIN_WEIGHTS if kind == "random" else (1,):
        vert, tri = GM.check(inst, v, words, mw, f"{GL.TWO_TILE_LAYER} {kind}, min_weight {mw}")
        assert len(tri) > 100


def small_volume_both_lists(inst, label):
    v, words = random_volume((3, 3, 2), 31, heavy=True)
    GM.check(inst, v, words, 1, label)
    pts = VR.crossings(words, v, 1)
    GV.same_list(label, GV.Device(v, words).extract(inst, 1, len(pts) + 2, label), pts)


def test_one_instance_through_the_big_volume_a_tiny_one_and_the_layer_of_two_tiles(big):
    """the tile scratch is reused: nothing of the scratch of 4128 tiles may show through a later, smaller mesh or list"""
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    try:
        want = GL.big_mesh(1)
        nv, nt, vert, tri = big[2].mesh(i, 1, len(want[0]) + 2, len(want[1]) + 2, "step 0: big")
        same_mesh("step 0: big", (vert, tri), want)
        GV.same_list("step 0: big points", big_points_once(i, big, 1, len(GL.big_points(1)) + 2, "step 0: big points"), GL.big_points(1))
        small_volume_both_lists(i, "step 1: 3x3x2")
        for kind in ("sphere", "random"):
            GM.check(i, *GL.two_tile_layer(kind), 1, f"step 2: {kind}")
        small_volume_both_lists(i, "step 3: 3x3x2 again")
    finally:
        i.close()


def test_under_guard_bands(big, monkeypatch):
    """the debug allocation mode around the tile scratch of 4128 tiles (two sets of words for the mesh) and of 4100 tiles of a
    cloud: the host's sizing at many tiles"""
    import torch
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(1 << 20))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    i = S.SGMInstance(0)
    try:
        want = GL.big_mesh(1)
        nv, nt, vert, tri = big[2].mesh(i, 1, len(want[0]) + 2, len(want[1]) + 2, "guarded big mesh")
        same_mesh("guarded big mesh", (vert, tri), want)
        s, disp, mask, conf, keep = GL.cloud_batch("one full tile a frame", "share 0.5")
        assert GC.check(i, s, disp, mask, conf, "guarded cloud of 4100 frames") == keep.sum()
        torch.cuda.synchronize()
        bad, live, size = S.debug_guard_check()
        assert bad == 0 and live > 0 and size > 0
    finally:
        i.close()
    assert S.debug_guard_check() == (0, 0, 0)


def test_integration_with_all_64_pose_slots_equals_64_calls_of_one_frame(inst):
    v, s, poses, disp = GL.integrate_case()
    want, updates = VR.integrate(VR.empty(v), v, s, poses, disp)
    batch = GV.integrate(inst, GV.Device(v), s, poses, disp, label="64 frames")
    GV.same_volume("64 frames", batch, want)
    dev = GV.Device(v)
    one = type(s)(**dict(vars(s), frames=1))
    for f in range(s.frames):
        single = GV.integrate(inst, dev, one, poses[f:f + 1], disp[f:f + 1], label=f"frame {f}")
    assert single.tobytes() == batch.tobytes()
    assert updates > 64 * 1000


# ---- slivers elsewhere ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_raycast_views_65535_wide_or_tall(inst, size):
    v, vox, vw, poses = GL.raycast_sliver(size)
    want_d, want_n, stats = GL.raycast_sliver_want(size)
    for skew in (False, True):
        depth, normal = GRC.render(inst, v, vox, vw, poses, f"ray-cast {size} skew={skew}", skew=skew)
        same_maps(f"ray-cast {size} depth", depth, want_d)
        same_maps(f"ray-cast {size} normal", normal, want_n)


@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_track_model_maps_65535_wide_or_tall(inst, size):
    s, disp, m, poses, depth, normal = GL.track_sliver(size)
    got = device_sums(inst, s, m, poses, Inputs(disp, depth, normal), f"track model {size}")
    want = GL.track_sliver_sums(size)
    assert got.tolist() == want.tolist() and want[0, 28] > 1000


@pytest.mark.parametrize("splat", [1, 2])
@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_register_targets_65535_wide_or_tall(inst, size, splat):
    s, r, disp, mask, conf = GL.register_target_sliver(size, splat)
    GG.check(inst, s, r, disp, mask, conf, f"register target {size} splat {splat}", GL.register_want("target", size, splat))


@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_register_sources_65535_wide_or_tall(inst, size):
    s, r, disp, mask, conf = GL.register_source_sliver(size)
    want = GL.register_want("source", size)
    GG.check(inst, s, r, disp, mask, conf, f"register source {size}", want)
    GG.check(inst, s, r, disp, mask, conf, f"register source {size} all off", want, misalign=True, skew_sides=True, skew_out=True)
