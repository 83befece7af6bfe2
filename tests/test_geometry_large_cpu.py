"""The cases of tests/geometry_large.py on the restatements alone: every case reaches the code it is for.  A case that stops short of
its loop, its chunk or its far tile is worthless on the device however green it is there, so each condition is an assertion here:
what a kernel that never went round again, a scan that lost its carry or a search that looked one tile too near would return is
computed with the restatements and differs from the truth.  Nothing here needs a GPU; test_gpu_geometry_large.py runs the same
cases through the library."""
import numpy as np
import pytest

import cloud_ref as CR
import geometry_large as GL
import mesh_ref as MR
import register_ref as GR
import track_ref as TR
import volume_ref as VR


# ---- the constants and the shapes that follow from them -----------------------------------------------------------------------

def test_the_constants_are_read_from_the_sources_and_give_todays_shapes():
    assert (GL.TRACK_MAX_BLOCKS, GL.TRACK_THREADS, GL.TILE_MAX, GL.SCAN_THREADS, GL.SCAN_PER_THREAD) == (128, 256, 2048, 1024, 4)
    assert list(GL.TRACK_SHAPES.values()) == [(257, 129, 1), (512, 258, 4), (520, 254, 4), (257, 161, 1), (512, 320, 4)]
    assert GL.TRACK_BIG == (1024, 512)
    assert list(GL.CLOUD_BATCHES.values()) == [(2, 2, 4100), (3, 1, 4099), (2049, 1, 2050)]
    assert GL.BIG_DIMS == (256, 192, 172) and GL.TWO_TILE_LAYER == (64, 64, 8) and GL.POSE_SLOTS == 64


# ---- track ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GL.TRACK_SHAPES))
def test_track_frames_go_round_the_grid_again(name):
    """more lane items than TRACK_MAX_BLOCKS workgroups hold; pixels beyond the first lap contribute in every frame; and the sums
    of the first lap alone -- what a kernel without its stride loop returns -- differ from the full ones in all 29 entries"""
    w, h, per_lane = GL.TRACK_SHAPES[name]
    items = w * h // per_lane
    assert GL.TRACK_LAP < items <= 2 * GL.TRACK_LAP
    quota = GL.track_quota(w, h, per_lane)
    assert quota == GL.TRACK_QUOTA or 4 * (w * h - GL.TRACK_LAP * per_lane) < GL.TRACK_LAP      # short of it only by the shape's own size
    for sides in (True, False):
        full, first = GL.track_want(name, sides), GL.track_want(name, sides, first_lap=per_lane)
        beyond = full[:, 28] - first[:, 28]
        print(f"{name} {w}x{h} side maps={sides}: {w * h - GL.TRACK_LAP * per_lane} pixels beyond the first lap, contributing {beyond.tolist()} "
              f"of {full[:, 28].tolist()}")
        assert full.shape == (GL.TRACK_FRAMES, 29) and np.all(beyond >= quota), (name, sides, beyond, quota)
        assert np.all(full != first), (name, sides)
    assert not np.array_equal(GL.track_want(name, True), GL.track_want(name, False))
    s, _, _, poses, *_ = GL.track_case(name)
    assert len({p.tobytes() for p in poses}) == s.frames == GL.TRACK_FRAMES


def test_track_the_skewed_run_takes_five_laps_of_one_pixel():
    w, h, per_lane = GL.TRACK_SHAPES[GL.TRACK_SKEWED]
    assert per_lane == 4 and 4 * GL.TRACK_LAP < w * h < 5 * GL.TRACK_LAP
    for sides in (True, False):
        full, first = GL.track_want(GL.TRACK_SKEWED, sides), GL.track_want(GL.TRACK_SKEWED, sides, first_lap=1)
        assert np.all(full[:, 28] - first[:, 28] >= GL.TRACK_QUOTA) and np.all(full != first)


def test_track_sums_leave_53_bits():
    s, disp, m, poses, depth, normal = GL.track_big()
    assert (s.width, s.height, s.frames) == GL.TRACK_BIG + (1,) and s.width * s.height == 4 * 4 * GL.TRACK_LAP
    want = GL.track_big_want()
    top = max(abs(int(v)) for v in want[0])
    print(f"{s.width}x{s.height}, span {m.span}: {int(want[0, 28])} contributing pixels, the largest sum takes {top.bit_length()} bits")
    assert top >= 1 << 53
    assert any(int(np.float64(int(v))) != int(v) for v in want[0])          # a sum that a double on the way would round
    # ... and the host's solve of these sums moves the pose
    step, stats = TR.solve(m, want[0], np.asarray(poses[0], np.float64))
    assert stats["status"] == 0 and step != [float(x) for x in poses[0]]


# ---- cloud ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", GL.CLOUD_VARIANTS)
@pytest.mark.parametrize("name", list(GL.CLOUD_BATCHES))
def test_cloud_batches_take_the_scan_into_a_second_chunk(name, variant):
    w, h, frames = GL.CLOUD_BATCHES[name]
    s, disp, mask, conf, keep = GL.cloud_batch(name, variant)
    tile, per_frame = GL.cloud_tiling(w, h)
    ntiles = per_frame * frames
    assert GL.CHUNK < ntiles <= GL.CHUNK + GL.SCAN_PER_THREAD
    assert np.array_equal(CR.kept(disp, s, mask, conf)[0].reshape(-1), keep)               # the maps do what the pattern says
    kept = GL.tile_counts(keep, w, h, frames)
    assert kept.sum() == keep.sum() and len(kept) == ntiles
    low, high = int(kept[:GL.CHUNK].sum()), int(kept[GL.CHUNK:].sum())
    print(f"{name} {w}x{h}x{frames} {variant}: tiles of {tile}, {ntiles} of them, kept {low} below tile {GL.CHUNK} and {high} from it on")
    assert high > 0
    if variant == "first chunk empty":
        assert low == 0 and not kept[:GL.CHUNK].any()
    elif variant == "first chunk full":
        assert low == (GL.cloud_tile_of(w, h, frames) < GL.CHUNK).sum() and np.all(keep[GL.cloud_tile_of(w, h, frames) < GL.CHUNK])
    else:
        assert low > 0
    # the offsets: base of every frame's first tile, then the total; with the carry dropped they differ wherever it is not zero
    true, lost = GL.tile_bases(kept), GL.tile_bases(kept, carry=False)
    first_tiles = np.arange(frames) * per_frame
    want_off = CR.points(disp, s, mask, conf)[1]
    assert np.array_equal(np.r_[true[first_tiles], kept.sum()], want_off)
    assert (first_tiles >= GL.CHUNK).any()                                                  # a frame whose offsets word the later chunk writes
    if variant == "first chunk empty":
        assert np.array_equal(true, lost)                                                   # the carry is zero going in
    else:
        assert np.all(true[first_tiles[first_tiles >= GL.CHUNK]] != lost[first_tiles[first_tiles >= GL.CHUNK]])
    if name == "two tiles a frame":                                                         # the frame boundary is not the chunk boundary
        assert per_frame == 2 and GL.CHUNK % per_frame == 0 and kept[GL.CHUNK + 1:].sum() > 0


@pytest.mark.parametrize("size", GL.CLOUD_SLIVERS, ids=GL.sliver_name)
def test_cloud_slivers_reach_the_top_pixel_word(size):
    w, h = size
    s, disp, mask, conf, keep = GL.cloud_sliver(w, h)
    pts, off = CR.points(disp, s, mask, conf)
    top = (h - 1) << 16 | (w - 1)
    assert int(pts["pixel"][-1]) == top and top in (0xFFFE0000, 0x0000FFFE) and int(pts["pixel"][0]) == 0
    assert off[-1] == keep.sum() > 30000


# ---- volume --------------------------------------------------------------------------------------------------------------------

def test_big_volume_has_records_on_both_sides_of_the_chunk_and_triangles_across_it():
    v, words = GL.big_volume()
    n = v.nx * v.ny * v.nz
    ntiles = -(-n // GL.TILE_MAX)
    assert GL.CHUNK < ntiles and GL.CHUNK * GL.TILE_MAX // (v.nx * v.ny) == v.nz - 2        # tile CHUNK starts in the last layer with cells
    lists = {}
    for mw in GL.MIN_WEIGHTS:
        vert, tri = GL.big_mesh(mw)
        pts = GL.big_points(mw)
        cell, home = GL.home_tiles(vert, tri)
        v_home, p_home = (vert["id"].astype(np.int64) >> 3) // GL.TILE_MAX, (pts["id"].astype(np.int64) >> 2) // GL.TILE_MAX
        print(f"{GL.BIG_DIMS} in {ntiles} tiles, min_weight {mw}: {len(vert)} vertices ({(v_home >= GL.CHUNK).sum()} from tile {GL.CHUNK} on), "
              f"{len(tri)} triangles ({(cell >= GL.CHUNK).sum()}), {len(pts)} surface points ({(p_home >= GL.CHUNK).sum()}); "
              f"{((cell < GL.CHUNK) & (home.max(axis=1) >= GL.CHUNK)).sum()} triangles below it with a vertex beyond; the furthest vertex "
              f"{(home.max(axis=1) - cell).max()} tiles up")
        for where in (v_home, cell, p_home):
            assert (where < GL.CHUNK).any() and (where >= GL.CHUNK).any()
        assert ((cell < GL.CHUNK) & (home.max(axis=1) >= GL.CHUNK)).any()
        assert (home.max(axis=1) - cell).max() >= v.nx * v.ny // GL.TILE_MAX                # z-neighbours a whole layer of tiles up
        lists[mw] = (vert, tri, pts)
    (v1, t1, p1), (v2, t2, p2) = lists[1], lists[2]
    assert 0 < len(v2) < len(v1) and 0 < len(t2) < len(t1) and 0 < len(p2) < len(p1)
    assert len(v1) > 100000 and len(t2) > 10000
    tq, w = VR.unpack(words)
    assert set(np.unique(w)) == {1, 2}


@pytest.mark.parametrize("kind", ["sphere", "random"])
def test_a_layer_of_two_tiles_puts_the_upper_corners_two_tiles_away(kind):
    v, words = GL.two_tile_layer(kind)
    assert v.nx * v.ny == 2 * GL.TILE_MAX
    vert, tri = MR.mesh(words, v, 1)
    cell, home = GL.home_tiles(vert, tri)
    far = (home.max(axis=1) - cell >= 2).sum()
    print(f"{GL.TWO_TILE_LAYER} {kind}: {len(vert)} vertices, {len(tri)} triangles, {far} with a vertex two or more tiles above the cell")
    assert far > 0 and len(tri) > (100 if kind == "sphere" else 10000)


def test_integration_uses_the_last_pose_slot():
    v, s, poses, disp = GL.integrate_case()
    assert s.frames == GL.POSE_SLOTS == len(poses)
    last = GL.POSE_SLOTS - 1
    one = lambda f: type(s)(**dict(vars(s), frames=f))
    before, _ = VR.integrate(VR.empty(v), v, one(last), poses[:last], disp[:last])
    want, updates = VR.integrate(VR.empty(v), v, s, poses, disp)
    changed = int((before != want).sum())
    swap = poses.copy()
    swap[[last - 1, last]] = swap[[last, last - 1]]
    swapped, _ = VR.integrate(VR.empty(v), v, s, swap, disp)
    print(f"64 frames: {updates} updates, frame 63 changes {changed} words, its pose swapped with frame 62's {int((swapped != want).sum())}")
    assert changed >= 1 and not np.array_equal(swapped, want)
    assert VR.unpack(want)[1].max() == GL.POSE_SLOTS                                        # a voxel every frame saw


# ---- slivers elsewhere ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_raycast_slivers_hit_at_both_ends(size):
    depth, normal, stats = GL.raycast_sliver_want(size)
    far, near = GL.ends_of(depth[0], *size)
    print(f"ray-cast {size}: {stats}, hits in the last {GL.EDGE}: {np.isfinite(far).sum()}, in the first: {np.isfinite(near).sum()}")
    assert np.isfinite(far).any() and np.isfinite(near).any() and stats["hits"] > 30000 and stats["normals"] > 30000


@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_track_slivers_associate_at_both_ends(size):
    s, disp, m, poses, depth, normal = GL.track_sliver(size)
    assert (m.width, m.height) == size
    total, far, near = (int(GL.track_sliver_sums(size, part)[0, 28]) for part in (None, "far", "near"))
    print(f"track model {size}: {total} associated, {far} in the last {GL.EDGE}, {near} in the first")
    assert total > GL.SLIVER_SOURCE // 2 and far >= 1 and near >= 1


@pytest.mark.parametrize("splat", [1, 2])
@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_register_target_slivers_are_hit_at_both_ends(size, splat):
    s, r, *_ = GL.register_target_sliver(size, splat)
    assert (r.width, r.height) == size
    depth, source = GL.register_want("target", size, splat)
    far, near = GL.ends_of(source, *size)
    print(f"register target {size} splat {splat}: {(source != GR.NONE).sum()} hit, {(far != GR.NONE).sum()} in the last {GL.EDGE}, "
          f"{(near != GR.NONE).sum()} in the first")
    assert (far != GR.NONE).any() and (near != GR.NONE).any() and (source != GR.NONE).sum() >= 2 * 60 * splat


@pytest.mark.parametrize("size", GL.SLIVERS, ids=GL.sliver_name)
def test_register_source_slivers_carry_the_top_column_or_row(size):
    s, r, *_ = GL.register_source_sliver(size)
    assert (s.width, s.height) == size
    depth, source = GL.register_want("source", size)
    won = source[source != GR.NONE].astype(np.int64)
    along = won & 0xFFFF if size[0] > size[1] else won >> 16
    print(f"register source {size}: {len(won)} winners, source pixels {along.min()} .. {along.max()}")
    assert len(won) > GL.SLIVER_SOURCE // 2 and along.max() >= 65535 - GL.EDGE and along.min() < GL.EDGE
