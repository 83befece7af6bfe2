"""The geometry kernels (cloud, register, volume, ray-cast, track, mesh) beyond one lap of the tracking grid, one chunk of the tile
scan and one tile's distance in the mesh's vertex search, and at the ends of the admitted image sizes: the cases as builders.  A
plain helper module, no fixtures; shared by test_geometry_large_cpu.py (the conditions: every case reaches the code it is for, on
the restatements alone) and test_gpu_geometry_large.py (the library against the restatements, byte for byte).

The shapes are derived from the constants of the sources, read with a regular expression: each is the smallest shape that reaches
what its comment names.  If a constant changes, the shapes follow, and the conditions of test_geometry_large_cpu.py still decide
whether a case reaches what it is for.  What the restatements make of every case is cached here, read-only, so that the tests
of a run share it.  NOTES.md has the table of shapes, counts and wall times."""
import functools
import os
import re

import numpy as np

import cloud_ref as CR
import mesh_ref as MR
import raycast_ref as RR
import register_ref as GR
import track_ref as TR
import volume_ref as VR
import test_gpu_cloud as GC
import test_gpu_register as GG
from test_mesh_cpu import random_volume
from test_raycast_cpu import noisy_volume
from test_track_cpu import IDENTITY, corner_seen, noisy_case
from test_volume_cpu import camera, noisy_maps, rot

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "soc_project_stereo_matching_amd", "csrc")
INF = np.float32(np.inf)
EDGE = 64                                                         # "the first / last 64 columns or rows" of a sliver


def constant(source, name):
    """#define `name` <integer> of csrc/`source`"""
    with open(os.path.join(CSRC, source)) as f:
        found = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)\b" % re.escape(name), f.read(), re.M)
    assert len(found) == 1, (source, name, found)
    return int(found[0])


TRACK_MAX_BLOCKS = constant("sgm_track.hip", "TRACK_MAX_BLOCKS")
TRACK_THREADS = constant("sgm_track.hip", "TRACK_THREADS")
TILE_MAX = constant("sgm_cloud_common.hpp", "TILE_MAX")
SCAN_THREADS = constant("sgm_cloud_common.hpp", "SCAN_THREADS")
SCAN_PER_THREAD = constant("sgm_cloud_common.hpp", "SCAN_PER_THREAD")
TRACK_LAP = TRACK_MAX_BLOCKS * TRACK_THREADS                      # the lane items (of one or four pixels) one lap of a frame's grid takes
CHUNK = SCAN_THREADS * SCAN_PER_THREAD                            # the tiles tile_scan takes before it carries


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def smallest(start, ok, step=1):
    n = start
    while not ok(n):
        n += step
    return n


# ================================================================================================ track: beyond the first lap
# name -> (w, h, pixels a lane takes where the maps are aligned).  A frame is odd (one pixel per lane) or a multiple of four.
def _track_shapes():
    t, lap = TRACK_THREADS, TRACK_LAP
    w1, w4, w4p = t + 1, 2 * t, 2 * t + 8
    out = {
        # the second lap's only workgroup is partial: the smallest odd frame of width t + 1 past one lap
        "scalar, a partial workgroup more": (w1, smallest(1, lambda h: w1 * h > lap and w1 * h % 2 == 1), 1),
        # one full workgroup of a second lap
        "four, one workgroup more": (w4, smallest(1, lambda h: w4 // 4 * h >= lap + t), 4),
        # a partial one, with lanes in all of its waves and a partial last wave
        "four, a partial workgroup more": (w4p, smallest(1, lambda h: lap + t - 64 < w4p // 4 * h < lap + t), 4),
        # a quarter of the second lap on either path: room for the quota of contributing pixels beyond the first lap
        "scalar, a quarter lap more": (w1, smallest(1, lambda h: 4 * w1 * h >= 5 * lap and w1 * h % 2 == 1), 1),
        "four, a quarter lap more": (w4, smallest(1, lambda h: 4 * (w4 // 4 * h) >= 5 * lap), 4),
    }
    for w, h, v in out.values():
        assert (w * h % 4 == 0) == (v == 4)
    return out


TRACK_SHAPES = _track_shapes()
TRACK_SKEWED = "four, one workgroup more"                         # also run one element off a 16-byte boundary: one pixel per lane, five laps
TRACK_FRAMES = 3
# Contributing pixels beyond the first lap, in every frame: 1000 where a quarter lap of them exists.  The partial workgroups of the
# first three shapes hold 385 to 1024 pixels in all; noisy_case drops about a third of a frame's pixels by its maps (0.95 finite,
# 0.85 masked in, 0.85 confident), a tenth by the model's (0.95 * 0.98^3), and the gates take more: a quarter of them is asked for.
TRACK_QUOTA = 1000
TRACK_BIG = (4 * TRACK_THREADS, 4 * TRACK_MAX_BLOCKS)             # four laps of four pixels per lane
TRACK_BIG_SPAN = 0.25                                             # |q_0..2| grows with 1 / span


def track_quota(w, h, per_lane):
    beyond = w * h - TRACK_LAP * per_lane
    return min(TRACK_QUOTA, beyond // 4)


@functools.lru_cache(maxsize=None)
def track_case(name):
    """(s, disp, m, poses, depth, normal, mask, conf) of noisy_case at the shape, three frames with three poses"""
    w, h, _ = TRACK_SHAPES[name]
    s, *arrays = noisy_case(seed=500 + w + h, frames=TRACK_FRAMES, w=w, h=h)
    return (s,) + frozen(*arrays)


def first_lap_only(disp, frames, per_lane):
    """the maps with every pixel beyond the first lap of a frame dropped: what a kernel that never went round again would sum"""
    cut = np.array(disp, np.float32).reshape(frames, -1)
    cut[:, TRACK_LAP * per_lane:] = INF
    return cut.reshape(np.shape(disp))


@functools.lru_cache(maxsize=None)
def track_want(name, sides, first_lap=0):
    """TR.sums of a case, with or without side maps; first_lap: restricted to the first lap of lanes taking that many pixels"""
    s, disp, m, poses, depth, normal, mask, conf = track_case(name)
    if first_lap:
        disp = first_lap_only(disp, s.frames, first_lap)
    return frozen(TR.sums(disp, s, m, poses, depth, normal, mask if sides else None, conf if sides else None))[0]


@functools.lru_cache(maxsize=None)
def track_big():
    """one frame of TRACK_BIG with span TRACK_BIG_SPAN, no side maps: (s, disp, m, poses, depth, normal).  (The seed: one whose two
    sums of 54 bits are odd, so that no double holds them; with others they happen to be even.)"""
    w, h = TRACK_BIG
    s, disp, m, poses, depth, normal, _, _ = noisy_case(seed=14, frames=1, w=w, h=h)
    m.span = TRACK_BIG_SPAN
    return (s,) + frozen(disp) + (m,) + frozen(poses, depth, normal)


@functools.lru_cache(maxsize=None)
def track_big_want():
    s, disp, m, poses, depth, normal = track_big()
    return frozen(TR.sums(disp, s, m, poses, depth, normal))[0]


# ================================================================================================ cloud: beyond one chunk of the scan
# name -> (w, h, frames)
CLOUD_BATCHES = {
    # a tile is a frame, four pixels per lane; the later chunk holds one thread's SCAN_PER_THREAD tiles
    "one full tile a frame": (2, 2, CHUNK + SCAN_PER_THREAD),
    # a partial tile a frame, one pixel per lane; the later chunk holds less than one thread takes
    "one partial tile a frame": (3, 1, CHUNK + SCAN_PER_THREAD - 1),
    # two tiles a frame, the second of one pixel: tile CHUNK is the first of frame CHUNK / 2, whose offsets word the later chunk writes
    "two tiles a frame": (TILE_MAX + 1, 1, CHUNK // 2 + 2),
}
CLOUD_VARIANTS = ("share 0.5", "every 65th", "first chunk empty", "first chunk full")
CLOUD_SLIVERS = [(65535, 1), (1, 65535)]


def cloud_tiling(w, h):
    """(tile, tiles per frame): tile_size and cloud_tiling of the sources"""
    npx, tile = w * h, 1
    while tile < TILE_MAX and tile < npx:
        tile <<= 1
    return tile, -(-npx // tile)


def cloud_tile_of(w, h, frames):
    """the tile of every pixel of the batch, in raster order"""
    tile, per_frame = cloud_tiling(w, h)
    p = np.arange(w * h, dtype=np.int64)
    return (np.arange(frames, dtype=np.int64)[:, None] * per_frame + (p // tile)[None, :]).reshape(-1)


@functools.lru_cache(maxsize=None)
def cloud_batch(name, variant):
    """(s, disp, mask, conf, keep): maps that keep exactly `keep` (test_gpu_cloud.maps_for).  "every 65th" counts from the batch's
    last pixel, so that the last tile, beyond the chunk, holds one; the "first chunk" variants are "share 0.5" with the first CHUNK
    tiles emptied or filled"""
    w, h, frames = CLOUD_BATCHES[name]
    n = w * h * frames
    rng = np.random.default_rng(1000 * w + frames + CLOUD_VARIANTS.index(variant))
    if variant == "every 65th":
        keep = (n - 1 - np.arange(n)) % 65 == 0
    else:
        keep = rng.random(n) < 0.5
        if variant != "share 0.5":
            keep[cloud_tile_of(w, h, frames) < CHUNK] = variant == "first chunk full"
    disp, mask, conf = GC.maps_for(keep, (frames, h, w), rng, non_finite=variant == "share 0.5")
    return (GC.make_spec(w, h, frames),) + frozen(disp, mask, conf, keep)


def tile_counts(keep, w, h, frames):
    """kept[tile] as sgm_cloud_count_k leaves it"""
    _, per_frame = cloud_tiling(w, h)
    return np.bincount(cloud_tile_of(w, h, frames), weights=np.asarray(keep).reshape(-1), minlength=per_frame * frames).astype(np.int64)


def tile_bases(kept, carry=True):
    """base[tile] of tile_scan; carry False: every chunk scanned from zero, as a scan without its running carry would"""
    base = np.cumsum(kept) - kept
    if not carry:
        for c in range(CHUNK, len(kept), CHUNK):
            base[c:c + CHUNK] -= base[c]
    return base


@functools.lru_cache(maxsize=None)
def cloud_sliver(w, h):
    """(s, disp, mask, conf, keep): half of the pixels kept, the first and the last among them"""
    n = w * h
    rng = np.random.default_rng(w + 3)
    keep = rng.random(n) < 0.5
    keep[[0, n - 1]] = True
    disp, mask, conf = GC.maps_for(keep, (1, h, w), rng, non_finite=True)
    return (GC.make_spec(w, h),) + frozen(disp, mask, conf, keep)


# ================================================================================================ volume: beyond one chunk of tiles
def _big_dims():
    nx = TILE_MAX // 8
    ny = 3 * nx // 4                                              # a layer of 24 tiles: tile CHUNK starts inside a layer
    assert nx * ny % TILE_MAX == 0 and CHUNK * TILE_MAX % (nx * ny) != 0
    return nx, ny, CHUNK * TILE_MAX // (nx * ny) + 2              # that layer, and one above it for its cells' upper corners


BIG_DIMS = _big_dims()
TWO_TILE_LAYER = (int(round((2 * TILE_MAX) ** 0.5)),) * 2 + (8,)  # nx * ny is two tiles: the z-neighbours live two tiles up
assert TWO_TILE_LAYER[0] * TWO_TILE_LAYER[1] == 2 * TILE_MAX
MIN_WEIGHTS = (1, 2)


@functools.lru_cache(maxsize=None)
def big_volume():
    """(spec, words): the tilted plane of test_gpu_mesh's three-tile case through every layer of BIG_DIMS, weights 1 and 2 mixed
    (three in four are 2: one cell in ten counts at min_weight 2)"""
    nx, ny, nz = BIG_DIMS
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float32) + np.float32(0.5)
    tq = np.rint(np.clip((x - 9.3 * nx / 20 + 0.2 * y - 0.15 * z) / 3, -1, 1) * 32767).astype(np.int64)
    w = np.where(np.random.default_rng(10).random(tq.shape) < 0.75, 2, 1)
    return VR.spec(nx, ny, nz, 0.05, (-0.5, -0.4, 0.8), 0.15), frozen(VR.pack(tq, w))[0]


@functools.lru_cache(maxsize=None)
def big_mesh(min_weight):
    v, words = big_volume()
    return frozen(*MR.mesh(words, v, min_weight))


@functools.lru_cache(maxsize=None)
def big_points(min_weight):
    v, words = big_volume()
    return frozen(VR.crossings(words, v, min_weight))[0]


@functools.lru_cache(maxsize=None)
def two_tile_layer(kind):
    """(spec, words) of TWO_TILE_LAYER: "sphere" or "random" (random_volume(..., heavy=True))"""
    v, words = MR.sphere(TWO_TILE_LAYER) if kind == "sphere" else random_volume(TWO_TILE_LAYER, 77, heavy=True)
    return v, frozen(words)[0]


def home_tiles(vert, tri):
    """(the tile of every triangle's cell, the home tiles of its three vertices): tiles of TILE_MAX voxels"""
    return tri["cell"].astype(np.int64) // TILE_MAX, (vert["id"].astype(np.int64) >> 3)[tri["v"]] // TILE_MAX


# ---- integration with every pose slot in use -----------------------------------------------------------------------------------
POSE_SLOTS = constant("sgm_device.h", "SGMD_MAX_POSES")          # the frames one call of the integration admits


@functools.lru_cache(maxsize=None)
def integrate_case():
    """(v, s, poses, disp): POSE_SLOTS (64) frames of a 24 x 16 source into the 36 x 33 x 20 volume of test_gpu_volume.py, 64 different poses"""
    from test_gpu_volume import volume
    v = volume((36, 33, 20))
    s = camera(24, 16, frames=POSE_SLOTS)
    poses = np.stack([VR.pose(rot(k % 3, 0.002 * k - 0.06), (0.004 * (k % 7) - 0.012, 0.003 * (k % 5) - 0.006, 0.0005 * k))
                      for k in range(POSE_SLOTS)])
    assert len({p.tobytes() for p in poses}) == POSE_SLOTS
    return (v, s) + frozen(poses, noisy_maps(s, np.random.default_rng(64)))


# ================================================================================================ slivers elsewhere
SLIVERS = [(65535, 1), (1, 65535)]


def sliver_name(size):
    return "%dx%d" % size


def _ends(w, h):
    """slices of the last and of the first EDGE columns or rows of a [..][h][w] map"""
    if w > h:
        return (Ellipsis, slice(w - EDGE, w)), (Ellipsis, slice(0, EDGE))
    return (Ellipsis, slice(h - EDGE, h), slice(None)), (Ellipsis, slice(0, EDGE), slice(None))


def ends_of(a, w, h):
    """(the last EDGE columns or rows, the first) of a map [..][h][w]"""
    far, near = _ends(w, h)
    return a[far], a[near]


def raycast_sliver(size):
    """(v, vox, view, poses): the noisy volume of the ray-cast tests under a view whose long side spans the volume's face, so that
    both ends of the sliver meet the surface"""
    w, h = size
    v, vox = noisy_volume()
    long = max(w, h)
    # the surface near Z = 1.03 seen 0.77 to either side along x, 0.36 along y: inside what the scene's 70 x 33 camera filled
    f = long / (1.5 if w > h else 0.7)
    c = (long - 1) / 2.0
    vw = RR.view(w, h, f if w > h else 40.0, f if h > w else 40.0, c if w > h else 0.0, c if h > w else 0.0, 0.3, 1.6, 0.1)
    return v, vox, vw, VR.pose()[None]


@functools.lru_cache(maxsize=None)
def raycast_sliver_want(size):
    v, vox, vw, poses = raycast_sliver(size)
    depth, normal, stats = RR.raycast(vox, v, vw, poses)
    return frozen(depth, normal) + (stats,)


SLIVER_SOURCE = 2048                                              # pixels of the short camera that looks along a sliver


@functools.lru_cache(maxsize=None)
def track_sliver(size):
    """(s, disp, m, poses, depth, normal): a model of one row (or column) of `size` pixels that sees the room corner, and a source
    of one row (column) of SLIVER_SOURCE pixels with the same field of view, slightly moved: its pixels land all along the model"""
    w, h = size
    wide = w > h
    n, k = max(w, h), SLIVER_SOURCE
    fm, fs = 40.0 * n / 70.0, 40.0 * k / 70.0
    if wide:
        m = TR.model(n, 1, fm, fm, (n - 1) / 2.0, 0.0, 0.3, 4.0)
        s = CR.spec(k, 1, fx=fs, fy=fs, cx=(k - 1) / 2.0, cy=0.0, baseline=1.0)
    else:
        m = TR.model(1, n, fm, fm, 0.0, (n - 1) / 2.0, 0.3, 4.0)
        s = CR.spec(1, k, fx=fs, fy=fs, cx=0.0, cy=(k - 1) / 2.0, baseline=1.0)
    rng = np.random.default_rng(n + (1 if wide else 2))
    depth, normal = corner_seen(m.width, m.height, m.fx, m.fy, m.cx, m.cy)
    z, _ = corner_seen(s.width, s.height, s.fx, s.fy, s.cx, s.cy)
    disp = (CR.fb_of(s) / z).astype(np.float32)[None]
    disp = (disp + rng.uniform(-0.02, 0.02, disp.shape)).astype(np.float32)
    depth = (depth[None] + rng.uniform(-0.02, 0.02, (1,) + depth.shape)).astype(np.float32)
    normal = (normal[None] + rng.uniform(-0.1, 0.1, (1,) + normal.shape)).astype(np.float32)
    for a, value, stay in ((disp, INF, 2), (depth, np.nan, EDGE)):          # one in twenty dropped, but both ends of the sliver stay
        drop = rng.random(a.size) < 0.05
        drop[:stay] = drop[-stay:] = False
        a.reshape(-1)[drop] = value
    pose = np.array(IDENTITY, np.float32)
    pose[9 if wide else 10] = 0.0004                              # a shift along the sliver of less than a source pixel
    return (s,) + frozen(disp) + (m,) + frozen(pose[None], depth, normal)


def track_sliver_sums(size, part=None):
    """TR.sums of a track sliver; part "far" / "near": with the model's depth kept only in its last / first EDGE pixels"""
    s, disp, m, poses, depth, normal = track_sliver(size)
    if part:
        far, near = _ends(m.width, m.height)
        only = np.full_like(depth, np.nan)
        only[far if part == "far" else near] = depth[far if part == "far" else near]
        depth = only
    return TR.sums(disp, s, m, poses, depth, normal)


def _spread(n_from, n_to):
    """(scale, centre) that take the pixels 0 .. n_from - 1 of a camera with its centre at (n_from - 1) / 2 to 17 .. n_to - 18"""
    k = (n_to - 35.0) / (n_from - 1.0)
    return k, 17.0 + k * (n_from - 1) / 2.0


@functools.lru_cache(maxsize=None)
def register_target_sliver(size, splat):
    """(s, r, disp, mask, conf): a 70 x 33 x 2 source registered to a target of one row (column), whose long side its columns
    (rows) span from end to end; the other axis is squeezed into the one row (column) as test_gpu_register's "53x1" does"""
    w, h = size
    sw, sh, frames = (70, 33, 2) if w > h else (33, 70, 2)
    s = GG.source_spec(sw, sh, frames)
    if w > h:
        k, c = _spread(sw, w)
        r = GR.spec(w, 1, k * s.fx, 1e-3, c, 0.4, splat=splat)
    else:
        k, c = _spread(sh, h)
        r = GR.spec(1, h, 1e-3, k * s.fy, 0.4, c, splat=splat)
    return (s, r) + frozen(*GG.maps_for((frames, sh, sw), np.random.default_rng(w + splat)))


@functools.lru_cache(maxsize=None)
def register_source_sliver(size):
    """(s, r, disp, mask, conf): a source of one row (column) of 65535 pixels registered to a target of SLIVER_SOURCE pixels along
    it: 32 source pixels contend for a target pixel, and the winners' source words run up to the top column (row)"""
    w, h = size
    s = GG.source_spec(w, h, 1)
    if w > h:
        k, c = _spread(w, SLIVER_SOURCE)
        r = GR.spec(SLIVER_SOURCE, 1, k * s.fx, 1e-3, c, 0.4, splat=1)
    else:
        k, c = _spread(h, SLIVER_SOURCE)
        r = GR.spec(1, SLIVER_SOURCE, 1e-3, k * s.fy, 0.4, c, splat=1)
    return (s, r) + frozen(*GG.maps_for((1, h, w), np.random.default_rng(w + 9)))


@functools.lru_cache(maxsize=None)
def register_want(kind, size, splat=1):
    s, r, disp, mask, conf = register_target_sliver(size, splat) if kind == "target" else register_source_sliver(size)
    return frozen(*GR.register(disp, s, r, mask, conf))
