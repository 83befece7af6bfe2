"""ctypes mirror of include/sgm_mi355x.h.

``SGM`` wraps the reference-shaped global entry points (SGM_Initialize / SGM_Reset / SGM_Match,
reference SemiGlobalMatching.h:78-80); ``SGMInstance`` wraps the explicit-instance extension
(several frames in flight, device-resident buffers).  Names, argument meaning and the
True/False error behaviour follow the C interface one to one.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LOAD_LOCK = threading.Lock()

STAGE_NAMES = ["census_l", "census_r", "cost", "aggr", "disp_l", "disp_r", "after_lr", "after_speckle", "final"]
_STAGE_DTYPE = [np.uint32, np.uint32, np.uint8, np.uint16] + [np.float32] * 5
# stages outside STAGE_NAMES (read_stages() leaves them out: they exist only with hole filling on, set_fill_holes)
STAGE_FILLED, STAGE_FILL_CLASS = 9, 18
# after a match_both: the right view after the LR check / after speckle removal (both need keep_stages) / finished
STAGE_RIGHT_AFTER_LR, STAGE_RIGHT_AFTER_SPECKLE, STAGE_RIGHT_FINAL = 26, 27, 28
# the rectified left / right image (u8; they exist only with rectification on, set_rectify: read_stages() leaves them out)
STAGE_RECT_LEFT, STAGE_RECT_RIGHT = 19, 20
# the narrowed left / right image of a match on more than 8 bits per sample (u8; set_pixel_bits: read_stages() leaves them out)
STAGE_NARROW_LEFT, STAGE_NARROW_RIGHT = 21, 22
# the temporal filter (set_temporal): the map as it entered the filter (needs keep_stages), the history value hv (float32) and the
# validity bits hb (uint8) of the selected frame's stream; the same three for the right view after a match_both
STAGE_TEMPORAL_IN, STAGE_TEMPORAL_VALUE, STAGE_TEMPORAL_BITS = 29, 30, 31
STAGE_RIGHT_TEMPORAL_IN, STAGE_RIGHT_TEMPORAL_VALUE, STAGE_RIGHT_TEMPORAL_BITS = 32, 33, 34
# the decisions the temporal filter counts, in the order of its statistics
TEMPORAL_CLASSES = ("first", "smoothed", "replaced", "held", "invalid")
# the refinement's default parameters (SGM_REFINE_DEFAULT_* of include/sgm_mi355x.h)
REFINE_LAMBDA, REFINE_SIGMA, REFINE_ITERS = 16.0, 1.5, 1
# census kinds (SGM_CENSUS_* of include/sgm_mi355x.h) and the drivers' window for the symmetric kind
CENSUS_CENTRE, CENSUS_SYMMETRIC = 0, 1
CENSUS_SYMMETRIC_WINDOW = (7, 7)


class SGMOption(C.Structure):
    """Field-for-field the reference's SGMOption (SemiGlobalMatching.h:24-40), 28 bytes."""
    _fields_ = [
        ("num_paths", C.c_uint8),
        ("min_disparity", C.c_uint16),
        ("max_disparity", C.c_uint16),
        ("is_check_unique", C.c_bool),
        ("uniqueness_ratio", C.c_float),
        ("is_check_lr", C.c_bool),
        ("lrcheck_thres", C.c_float),
        ("is_remove_speckles", C.c_bool),
        ("min_speckle_area", C.c_uint16),
        ("p1", C.c_int16),
        ("p2_init", C.c_int16),
    ]


class SGMCloudSpec(C.Structure):
    """Field-for-field sgm_cloud_spec of include/sgm_mi355x.h: 48 bytes, every field 4 bytes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("frames", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("baseline", C.c_float), ("doffs", C.c_float),
        ("z_min", C.c_float), ("z_max", C.c_float),
        ("min_conf", C.c_uint32),
    ]


# sgm_point of include/sgm_mi355x.h: 16 bytes, pixel = (y << 16) | x
POINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("pixel", np.uint32)])


def cloud_spec(width, height, fx, fy, cx, cy, baseline, doffs=0.0, frames=1, z_min=0.0, z_max=float("inf"), min_conf=0) -> SGMCloudSpec:
    """A sgm_cloud_spec; the defaults keep every pixel with a finite positive depth."""
    return SGMCloudSpec(int(width), int(height), int(frames), fx, fy, cx, cy, baseline, doffs, z_min, z_max, int(min_conf))


class SGMRegisterSpec(C.Structure):
    """Field-for-field sgm_register_spec of include/sgm_mi355x.h: 104 bytes, every field 4 bytes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("dist", C.c_float * 5), ("R", C.c_float * 9), ("t", C.c_float * 3),
        ("z_min", C.c_float), ("z_max", C.c_float),
        ("splat", C.c_int32),
    ]


REGISTER_NONE = 0xFFFFFFFF                      # what sgm_register_depth's source holds where nothing landed


def register_spec(width, height, fx, fy, cx, cy, dist=(0.0,) * 5, R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), t=(0.0,) * 3,
                  z_min=0.0, z_max=float("inf"), splat=2) -> SGMRegisterSpec:
    """A sgm_register_spec: the target camera of sgm_register_depth.  R (3x3, row-major) and t take a point of the rectified
    reference camera into the target camera; the defaults are the same place and every finite positive depth."""
    dist, R, t = (np.asarray(v, np.float64).reshape(-1) for v in (dist, R, t))
    if (dist.size, R.size, t.size) != (5, 9, 3):
        raise ValueError("register_spec: dist has 5 coefficients, R is 3x3, t has 3 entries")
    return SGMRegisterSpec(int(width), int(height), fx, fy, cx, cy, (C.c_float * 5)(*dist), (C.c_float * 9)(*R), (C.c_float * 3)(*t),
                           z_min, z_max, int(splat))


def register_spec_raw(K, dist, R, width, height, splat=2) -> SGMRegisterSpec:
    """sgm_register_spec_raw: the target "back into the raw camera that rectify_maps(K, dist, R, Knew, ..) rectified" (host only);
    the source pinhole to pair with it is Knew's."""
    mats = [np.ascontiguousarray(m, np.float64).reshape(-1) for m in (K, dist, R)]
    if [m.size for m in mats] != [9, 5, 9]:
        raise ValueError("register_spec_raw: K and R are 3x3, dist has 5 coefficients")
    out = SGMRegisterSpec()
    if not load_library().sgm_register_spec_raw(*(m.ctypes.data for m in mats), int(width), int(height), int(splat), C.byref(out)):
        raise ValueError("sgm_register_spec_raw: a size outside 1..65535, a splat other than 1 or 2 or a non-finite input")
    return out


class SGMVolumeSpec(C.Structure):
    """Field-for-field sgm_volume_spec of include/sgm_mi355x.h: 36 bytes, every field 4 bytes."""
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
        ("voxel", C.c_float), ("origin", C.c_float * 3), ("trunc", C.c_float),
        ("max_weight", C.c_uint32),
    ]


SURFACE_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("id", np.uint32)])   # sgm_surface_point


MESH_VERTEX_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("id", np.uint32)])    # sgm_mesh_vertex
MESH_TRIANGLE_DTYPE = np.dtype([("v", np.uint32, (3,)), ("cell", np.uint32)])                                   # sgm_mesh_triangle


class SGMMeshVertex(C.Structure):                                 # ctypes mirror of sgm_mesh_vertex
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("id", C.c_uint32)]


class SGMMeshTriangle(C.Structure):                               # ctypes mirror of sgm_mesh_triangle
    _fields_ = [("v", C.c_uint32 * 3), ("cell", C.c_uint32)]


def volume_spec(nx, ny, nz, voxel, origin, trunc, max_weight=64) -> SGMVolumeSpec:
    """A sgm_volume_spec: nx x ny x nz voxels of edge `voxel` (units of baseline), the corner of voxel (0, 0, 0) at `origin` in the
    world, truncation distance `trunc`, weights capped at max_weight (1..65535)."""
    origin = np.asarray(origin, np.float64).reshape(-1)
    if origin.size != 3:
        raise ValueError("volume_spec: origin has 3 entries")
    return SGMVolumeSpec(int(nx), int(ny), int(nz), voxel, (C.c_float * 3)(*origin), trunc, int(max_weight))


def volume_bytes(spec: SGMVolumeSpec) -> int:
    """sgm_volume_bytes: the size of the volume's device array (uint32 per voxel), 0 for a spec outside its ranges (host only)."""
    return int(load_library().sgm_volume_bytes(C.byref(spec)))


class SGMVolumeBox(C.Structure):
    """Field-for-field sgm_volume_box of include/sgm_mi355x.h: a box of n voxels (its cells and one more) starting at lo; 24 bytes."""
    _fields_ = [("lo", C.c_int32 * 3), ("n", C.c_int32 * 3)]


def _int3(values, what):
    values = [int(x) for x in values]
    if len(values) != 3:
        raise ValueError(what + ": three integers")
    return (C.c_int32 * 3)(*values)


def volume_window_spec(src: SGMVolumeSpec, offset, dims):
    """sgm_volume_window_spec (host only): the spec of the window of `dims` voxels that starts `offset` voxels into `src`; None
    where sgm_volume_window would refuse the three."""
    dst = SGMVolumeSpec()
    ok = load_library().sgm_volume_window_spec(C.byref(src), _int3(offset, "volume_window_spec"), _int3(dims, "volume_window_spec"), C.byref(dst))
    return dst if ok else None


def volume_follow(spec: SGMVolumeSpec, pose, focus_z=0.0, granule=4, margin=0):
    """sgm_volume_follow (host only): the shift (sx, sy, sz) in voxels, a multiple of `granule` per axis, that brings the point
    (0, 0, focus_z) of the camera with the world -> camera `pose` back to the middle of the volume; 0 on an axis where it is within
    `margin` voxels of the middle.  None where the call refuses."""
    pose = np.ascontiguousarray(pose, np.float32).reshape(-1)
    if pose.size != 12:
        raise ValueError("volume_follow: one pose of 12 floats (R row-major, then t)")
    shift = (C.c_int32 * 3)()
    ok = load_library().sgm_volume_follow(C.byref(spec), pose.ctypes.data, float(focus_z), int(granule), int(margin), shift)
    return tuple(shift) if ok else None


def volume_leaving(spec: SGMVolumeSpec, shift):
    """sgm_volume_leaving (host only): the boxes [(lo, n), ...] of voxels, at most three, that `shift` drops from the volume, each
    to be handed to volume_window as (offset, dims); None where the call refuses."""
    boxes = (SGMVolumeBox * 3)()
    count = load_library().sgm_volume_leaving(C.byref(spec), _int3(shift, "volume_leaving"), boxes)
    return None if count < 0 else [(tuple(b.lo), tuple(b.n)) for b in boxes[:count]]


DISTANCE_FAR = 0xFFFF


class SGMDistanceSpec(C.Structure):
    """Field-for-field sgm_distance_spec of include/sgm_mi355x.h: 16 bytes, every field 4 bytes."""
    _fields_ = [("min_weight", C.c_uint32), ("radius", C.c_int32), ("side", C.c_int32), ("unknown", C.c_int32)]


def distance_spec(min_weight, radius, side=0, unknown=0) -> SGMDistanceSpec:
    """The sites and the radius of sgm_volume_distance: a voxel is observed iff its weight >= min_weight (1..65535); the obstacle
    set is the observed voxels with tq < 0, and with unknown == 1 the unobserved ones; side 0 measures to the obstacle set, side 1
    to its complement; radius 1..255 voxels, beyond which a voxel reads DISTANCE_FAR.  The library validates the values."""
    return SGMDistanceSpec(int(min_weight), int(radius), int(side), int(unknown))


def volume_distance_bytes(spec: SGMVolumeSpec) -> int:
    """sgm_volume_distance_bytes: 2 * nx * ny * nz, 0 for a spec the library refuses"""
    return int(load_library().sgm_volume_distance_bytes(C.byref(spec)))


class SGMRaycastSpec(C.Structure):
    """Field-for-field sgm_raycast_spec of include/sgm_mi355x.h: 44 bytes, every field 4 bytes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("frames", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("z_min", C.c_float), ("z_max", C.c_float), ("step", C.c_float),
        ("min_weight", C.c_uint32),
    ]


def raycast_spec(width, height, fx, fy, cx, cy, z_min, z_max, step, min_weight=1, frames=1) -> SGMRaycastSpec:
    """A sgm_raycast_spec: `frames` pinhole views of width x height, marched at Z = z_min + k * step while Z <= z_max (units of the
    volume); a voxel counts with a weight of at least min_weight (1..65535)."""
    return SGMRaycastSpec(int(width), int(height), int(frames), fx, fy, cx, cy, z_min, z_max, step, int(min_weight))


class SGMTrackSpec(C.Structure):
    """Field-for-field sgm_track_spec of include/sgm_mi355x.h: 44 bytes, every field 4 bytes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("dist_max", C.c_float), ("span", C.c_float),
        ("iterations", C.c_int32), ("min_pixels", C.c_uint32), ("min_pivot", C.c_float),
    ]


class SGMTrackStats(C.Structure):
    """sgm_track_stats of include/sgm_mi355x.h: 16 bytes; status 0 ok, 1 too few pixels, 2 degenerate."""
    _fields_ = [("rms", C.c_double), ("pixels", C.c_uint32), ("status", C.c_int32)]


def track_spec(width, height, fx, fy, cx, cy, dist_max, span, iterations=1, min_pixels=6, min_pivot=0.0) -> SGMTrackSpec:
    """A sgm_track_spec: the model maps' size and pinhole, the association gate dist_max (also the unit of the residual), the length
    `span` that normalises the rotational Jacobian (about the scene depth), the rounds of SGMInstance.track and the two thresholds
    of the solve."""
    return SGMTrackSpec(int(width), int(height), fx, fy, cx, cy, dist_max, span, int(iterations), int(min_pixels), min_pivot)


def track_solve(model: SGMTrackSpec, sums, pose):
    """sgm_track_solve (host only): one step from the 29 sums of a frame -> (the stepped pose, float64 [12], or `pose` where the
    status is not 0; a dict of pixels, rms and status).  None for a refused call."""
    sums = np.ascontiguousarray(sums, np.int64).reshape(-1)
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1)
    if sums.size != 29 or pose.size != 12:
        raise ValueError("track_solve: 29 sums and a pose of 12 doubles")
    out, st = np.empty(12, np.float64), SGMTrackStats()
    if not load_library().sgm_track_solve(C.byref(model), sums.ctypes.data, pose.ctypes.data, out.ctypes.data, C.byref(st)):
        return None
    return out, dict(pixels=int(st.pixels), rms=float(st.rms), status=int(st.status))


def track_world_pose(model_pose, rel):
    """sgm_track_world_pose (host only): rel^-1 o model_pose as float32 [12], the world -> camera pose of the tracked frame; None
    for a refused call."""
    model_pose = np.ascontiguousarray(model_pose, np.float32).reshape(-1)
    rel = np.ascontiguousarray(rel, np.float64).reshape(-1)
    if model_pose.size != 12 or rel.size != 12:
        raise ValueError("track_world_pose: two poses of 12 entries")
    out = np.empty(12, np.float32)
    if not load_library().sgm_track_world_pose(model_pose.ctypes.data, rel.ctypes.data, out.ctypes.data):
        return None
    return out


class SGMPlane(C.Structure):
    """sgm_plane of include/sgm_mi355x.h: 32 bytes; normal . (P - anchor) = 0, offset = -(normal . anchor); all-zero normal: void."""
    _fields_ = [("normal", C.c_float * 3), ("offset", C.c_float), ("anchor", C.c_float * 3), ("votes", C.c_uint32)]


PLANE_DTYPE = np.dtype([("normal", np.float32, (3,)), ("offset", np.float32), ("anchor", np.float32, (3,)), ("votes", np.uint32)])


class SGMPlaneSpec(C.Structure):
    """Field-for-field sgm_plane_spec of include/sgm_mi355x.h: 44 bytes, every field 4 bytes."""
    _fields_ = [
        ("hypotheses", C.c_int32), ("seed", C.c_uint32), ("dist", C.c_float), ("axis", C.c_float * 3), ("min_cos", C.c_float),
        ("span", C.c_float), ("iterations", C.c_int32), ("min_inliers", C.c_uint32), ("min_pivot", C.c_float),
    ]


class SGMPlaneStats(C.Structure):
    """sgm_plane_stats of include/sgm_mi355x.h: 16 bytes; status 0 ok, 1 too few inliers, 2 degenerate."""
    _fields_ = [("rms", C.c_double), ("inliers", C.c_uint32), ("status", C.c_int32)]


def plane_spec(hypotheses, dist, span, seed=0, axis=(0.0, 0.0, 0.0), min_cos=0.0, iterations=1, min_inliers=3, min_pivot=0.0) -> SGMPlaneSpec:
    """A sgm_plane_spec: the number of candidate planes of a vote and the seed of the hash that picks them, the inlier half-thickness
    dist, the orientation prior (axis all zero: none), the length `span` that normalises coordinates before they are quantised, the
    rounds of SGMInstance.plane_fit and the two thresholds of the solve."""
    return SGMPlaneSpec(int(hypotheses), int(seed) & 0xFFFFFFFF, dist, (C.c_float * 3)(*axis), min_cos, span, int(iterations),
                        int(min_inliers), min_pivot)


class SGMComponentSpec(C.Structure):
    """Field-for-field sgm_component_spec of include/sgm_mi355x.h: 168 bytes, every field 4 bytes."""
    _fields_ = [("min_weight", C.c_uint32), ("set", C.c_int32), ("unknown", C.c_int32), ("connectivity", C.c_int32),
                ("min_voxels", C.c_uint32), ("planes", C.c_int32), ("plane", SGMPlane * 4), ("clearance", C.c_float * 4)]


class SGMComponent(C.Structure):
    """sgm_component of include/sgm_mi355x.h: 48 bytes."""
    _fields_ = [("first", C.c_uint32), ("voxels", C.c_uint32), ("lo", C.c_uint16 * 3), ("hi", C.c_uint16 * 3), ("reserved", C.c_uint32),
                ("sum", C.c_uint64 * 3)]


COMPONENT_DTYPE = np.dtype([("first", np.uint32), ("voxels", np.uint32), ("lo", np.uint16, (3,)), ("hi", np.uint16, (3,)),
                            ("reserved", np.uint32), ("sum", np.uint64, (3,))])
assert COMPONENT_DTYPE.itemsize == 48 and C.sizeof(SGMComponent) == 48 and C.sizeof(SGMComponentSpec) == 168


def component_spec(min_weight, set=0, unknown=0, connectivity=6, min_voxels=1, planes=(), clearance=()) -> SGMComponentSpec:
    """A sgm_component_spec: the set whose components are labelled (set 0: observed voxels with tq < 0, 1: observed with tq >= 0;
    unknown 1: the unobserved ones as well), the connectivity (6 or 26), the smallest component that keeps its label, and up to four
    planes (PLANE_DTYPE records) with a clearance each: a voxel whose centre lies at or below clearance along a plane's normal is
    taken out of the set.  The library validates the values; more than four planes are passed on by their number and refused."""
    planes = np.ascontiguousarray(planes, PLANE_DTYPE).reshape(-1) if len(planes) else np.zeros(0, PLANE_DTYPE)
    clearance = np.ascontiguousarray(clearance, np.float32).reshape(-1)
    if planes.size != clearance.size:
        raise ValueError("component_spec: one clearance per plane")
    sp = SGMComponentSpec(int(min_weight), int(set), int(unknown), int(connectivity), int(min_voxels), int(planes.size))
    for q in range(min(planes.size, 4)):
        sp.plane[q] = SGMPlane.from_buffer_copy(planes[q].tobytes())
        sp.clearance[q] = float(clearance[q])
    return sp


def volume_components_bytes(spec: SGMVolumeSpec) -> int:
    """sgm_volume_components_bytes: 4 * nx * ny * nz, the label array, 0 for a spec the library refuses"""
    return int(load_library().sgm_volume_components_bytes(C.byref(spec)))


def component_metric(spec: SGMVolumeSpec, obj):
    """sgm_component_metric (host only): the box corners and the centroid of one COMPONENT_DTYPE record in world units ->
    (lo, hi, centroid), float32 [3] each."""
    obj = np.ascontiguousarray(obj, COMPONENT_DTYPE).reshape(-1)
    if obj.size != 1:
        raise ValueError("component_metric: one record")
    out = np.zeros((3, 3), np.float32)
    load_library().sgm_component_metric(C.byref(spec), obj.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    return out[0], out[1], out[2]


def _plane_record(pl: SGMPlane) -> np.ndarray:
    return np.frombuffer(bytes(pl), PLANE_DTYPE)[0].copy()


def plane_solve(spec: SGMPlaneSpec, sums, plane):
    """sgm_plane_solve (host only): one round of the fit from the ten sums -> (the stepped plane, a PLANE_DTYPE record, or `plane`
    where the status is not 0; a dict of inliers, rms and status).  None for a refused call."""
    sums = np.ascontiguousarray(sums, np.int64).reshape(-1)
    plane = np.ascontiguousarray(plane, PLANE_DTYPE).reshape(-1)
    if sums.size != 10 or plane.size != 1:
        raise ValueError("plane_solve: 10 sums and one plane")
    out, st = SGMPlane(), SGMPlaneStats()
    if not load_library().sgm_plane_solve(C.byref(spec), sums.ctypes.data, plane.ctypes.data, C.byref(out), C.byref(st)):
        return None
    return _plane_record(out), dict(inliers=int(st.inliers), rms=float(st.rms), status=int(st.status))


class SGMScaleSpec(C.Structure):
    """Field-for-field sgm_scale_spec of include/sgm_mi355x.h: 36 bytes, every field 4 bytes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("frames", C.c_int32),
        ("factor", C.c_int32), ("bits", C.c_int32), ("radius", C.c_int32), ("penalty", C.c_int32),
        ("d_lo", C.c_int32), ("d_hi", C.c_int32),
    ]


SCALE_DEFAULT_RADIUS, SCALE_DEFAULT_PENALTY = 3, 1


class SGMTemporalSpec(C.Structure):
    """Field-for-field sgm_temporal_spec of include/sgm_mi355x.h: 28 bytes, every field 4 bytes."""
    _fields_ = [
        ("alpha", C.c_float), ("delta", C.c_float),
        ("hold_window", C.c_int32), ("hold_count", C.c_int32), ("sequence", C.c_int32),
        ("min_conf", C.c_uint32), ("stats", C.c_int32),
    ]


def temporal_spec(alpha=0.4, delta=1.0, hold_window=0, hold_count=1, sequence=False, min_conf=0, stats=False) -> SGMTemporalSpec:
    """A sgm_temporal_spec; the defaults smooth within one disparity and never bridge a hole."""
    return SGMTemporalSpec(alpha, delta, int(hold_window), int(hold_count), int(sequence), int(min_conf), int(stats))


def scale_spec(width, height, factor, frames=1, bits=8, radius=SCALE_DEFAULT_RADIUS, penalty=SCALE_DEFAULT_PENALTY, d_lo=0,
               d_hi=65535) -> SGMScaleSpec:
    """A sgm_scale_spec for FULL-resolution frames of width x height, matched at 1 / factor."""
    return SGMScaleSpec(int(width), int(height), int(frames), int(factor), int(bits), int(radius), int(penalty), int(d_lo), int(d_hi))


def scaled_shape(spec: SGMScaleSpec):
    """sgm_scaled_shape: (w, h) of the low-resolution frames, or None for a spec the library refuses.  Host only."""
    w, h = C.c_int(0), C.c_int(0)
    ok = load_library().sgm_scaled_shape(C.byref(spec), C.byref(w), C.byref(h))
    return (w.value, h.value) if ok else None


def default_option(max_disparity=64, min_disparity=0, **kw) -> SGMOption:
    """The option values the reference's driver sets (main.c:48-65), with overrides."""
    o = SGMOption()
    o.num_paths = 8
    o.min_disparity = min_disparity
    o.max_disparity = max_disparity
    o.is_check_lr = True
    o.lrcheck_thres = 1.0
    o.is_check_unique = True
    o.uniqueness_ratio = 0.99
    o.is_remove_speckles = True
    o.min_speckle_area = 50
    o.p1 = 10
    o.p2_init = 150
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def library_path() -> str:
    """The in-tree library; SGM_LIBRARY_PATH points experiments (tools/sweep_sched.sh) at another build of it."""
    return os.environ.get("SGM_LIBRARY_PATH") or os.path.join(_HERE, "libsgm_mi355x.so")


def load_library() -> C.CDLL:
    """Load libsgm_mi355x.so (built by csrc/Makefile or __graft_entry__.build()).  There is no
    fallback: a missing library is an error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOAD_LOCK:                                  # callers may be threads (ranks of a tile pipeline, host threads of a stream)
        if _LIB is None:
            _LIB = _load()
    return _LIB


def _load() -> C.CDLL:
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C soc_project_stereo_matching_amd/csrc` "
                           "(needs hipcc); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    L = C.CDLL(path)
    opt_p = C.c_void_p      # any ctypes structure with the SGMOption layout (28 bytes)
    for f in (L.SGM_Initialize, L.SGM_Reset):
        f.argtypes = [C.c_uint16, C.c_uint16, opt_p]
        f.restype = C.c_bool
    for f in (L.SGM_Match, L.SGM_MatchDevice):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_bool
    L.SGM_Synchronize.restype = C.c_bool
    L.SGM_SetDevice.argtypes = [C.c_int]
    L.SGM_SetDevice.restype = C.c_bool
    L.SGM_SetHonorNumPaths.argtypes = [C.c_int]
    L.SGM_KeepStages.argtypes = [C.c_int]
    L.SGM_ReadStage.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
    L.SGM_ReadStage.restype = C.c_size_t
    L.SGM_SynthPair.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    L.SGM_Version.restype = C.c_char_p
    L.sgm_create.argtypes = [C.c_int]
    L.sgm_create.restype = C.c_void_p
    L.sgm_destroy.argtypes = [C.c_void_p]
    L.sgm_set_honor_num_paths.argtypes = [C.c_void_p, C.c_int]
    L.sgm_set_overlap_post.argtypes = [C.c_void_p, C.c_int]
    L.sgm_set_overlap_post.restype = C.c_bool
    if hasattr(L, "sgm_set_stage_cus"):       # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_stage_cus.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.sgm_set_stage_cus.restype = C.c_bool
        L.sgm_set_stage_priority.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.sgm_set_stage_priority.restype = C.c_bool
    L.sgm_set_census_window.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.sgm_set_census_window.restype = C.c_bool
    L.sgm_set_reference_view.argtypes = [C.c_void_p, C.c_int]
    L.SGM_SetCensusWindow.argtypes = [C.c_int, C.c_int]
    L.SGM_SetCensusWindow.restype = C.c_bool
    L.SGM_SetReferenceView.argtypes = [C.c_int]
    if hasattr(L, "sgm_set_census_kind"):     # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_census_kind.argtypes = [C.c_void_p, C.c_int]
        L.sgm_set_census_kind.restype = C.c_bool
        L.SGM_SetCensusKind.argtypes = [C.c_int]
        L.SGM_SetCensusKind.restype = C.c_bool
    L.sgm_keep_stages.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "sgm_set_fill_holes"):      # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_fill_holes.argtypes = [C.c_void_p, C.c_int]
        L.sgm_set_fill_holes.restype = C.c_bool
        L.SGM_SetFillHoles.argtypes = [C.c_int]
        L.SGM_SetFillHoles.restype = C.c_bool
        L.sgm_fill_holes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sgm_fill_holes.restype = C.c_bool
    if hasattr(L, "sgm_set_refine"):          # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_refine.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
        L.sgm_set_refine.restype = C.c_bool
        L.SGM_SetRefine.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
        L.SGM_SetRefine.restype = C.c_bool
        L.sgm_refine_table.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
        L.sgm_refine_table.restype = C.c_bool
        L.sgm_refine_disparity.argtypes = [C.c_void_p] * 4
        L.sgm_refine_disparity.restype = C.c_bool
    if hasattr(L, "sgm_match_confidence"):    # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        for f in (L.sgm_match_confidence, L.sgm_match_confidence_async, L.sgm_match_confidence_device):
            f.argtypes = [C.c_void_p] * 5
            f.restype = C.c_bool
        L.SGM_MatchConfidence.argtypes = [C.c_void_p] * 4
        L.SGM_MatchConfidence.restype = C.c_bool
    if hasattr(L, "sgm_match_both"):          # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        for f in (L.sgm_match_both, L.sgm_match_both_async, L.sgm_match_both_device):
            f.argtypes = [C.c_void_p] * 5
            f.restype = C.c_bool
        L.SGM_MatchBoth.argtypes = [C.c_void_p] * 4
        L.SGM_MatchBoth.restype = C.c_bool
        L.sgm_depth_from_both.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_float] * 4 + [C.c_void_p]
        L.sgm_depth_from_both.restype = C.c_bool
    if hasattr(L, "sgm_set_rectify"):         # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_rectify.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.sgm_set_rectify.restype = C.c_bool
        L.SGM_SetRectify.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        L.SGM_SetRectify.restype = C.c_bool
        L.sgm_rectify.argtypes = [C.c_void_p] * 5
        L.sgm_rectify.restype = C.c_bool
        L.sgm_rectify_maps.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sgm_rectify_maps.restype = C.c_bool
    if hasattr(L, "sgm_match_scaled"):
        L.sgm_scaled_shape.argtypes = [C.c_void_p] * 3
        L.sgm_scaled_shape.restype = C.c_bool
        L.sgm_downscale.argtypes = [C.c_void_p] * 4
        L.sgm_downscale.restype = C.c_bool
        L.sgm_upscale_disparity.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        L.sgm_upscale_disparity.restype = C.c_bool
        L.sgm_match_scaled.argtypes = [C.c_void_p] * 5
        L.sgm_match_scaled.restype = C.c_bool
        L.sgm_match_scaled_device.argtypes = [C.c_void_p] * 5
        L.sgm_match_scaled_device.restype = C.c_bool
        L.SGM_MatchScaled.argtypes = [C.c_void_p] * 4
        L.SGM_MatchScaled.restype = C.c_bool
    if hasattr(L, "sgm_cloud_points"):        # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_cloud_organized.argtypes = [C.c_void_p] * 6
        L.sgm_cloud_organized.restype = C.c_bool
        L.sgm_cloud_points.argtypes = [C.c_void_p] * 7
        L.sgm_cloud_points.restype = C.c_bool
        L.sgm_read_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sgm_read_cloud.restype = C.c_bool
        L.SGM_ReadCloud.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.SGM_ReadCloud.restype = C.c_bool
        L.sgm_rectify_valid_mask.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sgm_rectify_valid_mask.restype = C.c_bool
    if hasattr(L, "sgm_register_depth"):      # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_register_depth.argtypes = [C.c_void_p] * 8
        L.sgm_register_depth.restype = C.c_bool
        L.sgm_register_gather.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
        L.sgm_register_gather.restype = C.c_bool
        L.sgm_register_spec_raw.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]
        L.sgm_register_spec_raw.restype = C.c_bool
    if hasattr(L, "sgm_volume_integrate"):    # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_bytes.argtypes = [C.c_void_p]
        L.sgm_volume_bytes.restype = C.c_size_t
        L.sgm_volume_integrate.argtypes = [C.c_void_p] * 8
        L.sgm_volume_integrate.restype = C.c_bool
        L.sgm_volume_points.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sgm_volume_points.restype = C.c_bool
    if hasattr(L, "sgm_volume_mesh"):         # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_mesh.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sgm_volume_mesh.restype = C.c_bool
    if hasattr(L, "sgm_volume_raycast"):      # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_raycast.argtypes = [C.c_void_p] * 7
        L.sgm_volume_raycast.restype = C.c_bool
    if hasattr(L, "sgm_volume_colors"):       # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_integrate_color.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p]
        L.sgm_volume_integrate_color.restype = C.c_bool
        L.sgm_volume_raycast_color.argtypes = [C.c_void_p] * 9
        L.sgm_volume_raycast_color.restype = C.c_bool
        L.sgm_volume_colors.argtypes = [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.sgm_volume_colors.restype = C.c_bool
    if hasattr(L, "sgm_volume_window"):       # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_window.argtypes = [C.c_void_p] * 9
        L.sgm_volume_window.restype = C.c_bool
        L.sgm_volume_window_spec.argtypes = [C.c_void_p] * 4
        L.sgm_volume_window_spec.restype = C.c_bool
        L.sgm_volume_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p]
        L.sgm_volume_follow.restype = C.c_bool
        L.sgm_volume_leaving.argtypes = [C.c_void_p] * 3
        L.sgm_volume_leaving.restype = C.c_int
    if hasattr(L, "sgm_volume_distance"):     # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_volume_distance_bytes.argtypes = [C.c_void_p]
        L.sgm_volume_distance_bytes.restype = C.c_size_t
        L.sgm_volume_distance.argtypes = [C.c_void_p] * 5
        L.sgm_volume_distance.restype = C.c_bool
        L.sgm_volume_distance_field.argtypes = [C.c_void_p] * 5
        L.sgm_volume_distance_field.restype = C.c_bool
    if hasattr(L, "sgm_volume_components"):   # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        _vp, _sz = C.c_void_p, C.c_size_t
        L.sgm_volume_components_bytes.argtypes = [_vp]
        L.sgm_volume_components_bytes.restype = _sz
        L.sgm_volume_components.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
        L.sgm_volume_components.restype = C.c_bool
        L.sgm_volume_component_of.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, C.c_int, _vp]
        L.sgm_volume_component_of.restype = C.c_bool
        L.sgm_component_metric.argtypes = [_vp] * 5
        L.sgm_component_metric.restype = None
    if hasattr(L, "sgm_plane_votes"):
        _vp, _sz = C.c_void_p, C.c_size_t
        L.sgm_plane_votes.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp]
        L.sgm_plane_best.argtypes = [_vp, _vp, C.c_int, _vp]
        L.sgm_plane_sums.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
        L.sgm_plane_label.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, C.c_int, _vp]
        L.sgm_plane_solve.argtypes = [_vp] * 5
        L.sgm_plane_fit.argtypes = [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]
        for name in ("votes", "best", "sums", "label", "solve", "fit"):
            getattr(L, "sgm_plane_" + name).restype = C.c_bool
    if hasattr(L, "sgm_track_sums"):          # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_track_sums.argtypes = [C.c_void_p] * 10
        L.sgm_track_sums.restype = C.c_bool
        L.sgm_track_solve.argtypes = [C.c_void_p] * 5
        L.sgm_track_solve.restype = C.c_bool
        L.sgm_track.argtypes = [C.c_void_p] * 12
        L.sgm_track.restype = C.c_bool
        L.sgm_track_world_pose.argtypes = [C.c_void_p] * 3
        L.sgm_track_world_pose.restype = C.c_bool
    if hasattr(L, "sgm_set_temporal"):        # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_temporal_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 5
        L.sgm_temporal_filter.restype = C.c_bool
        L.sgm_temporal_clear.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sgm_temporal_clear.restype = C.c_bool
        L.sgm_set_temporal.argtypes = [C.c_void_p, C.c_void_p]
        L.sgm_set_temporal.restype = C.c_bool
        L.sgm_temporal_restart.argtypes = [C.c_void_p]
        L.sgm_temporal_restart.restype = C.c_bool
        L.sgm_temporal_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.sgm_temporal_stats.restype = C.c_int
        L.SGM_SetTemporal.argtypes = [C.c_void_p]
        L.SGM_SetTemporal.restype = C.c_bool
        L.SGM_TemporalRestart.restype = C.c_bool
        L.SGM_TemporalStats.argtypes = [C.c_void_p, C.c_int]
        L.SGM_TemporalStats.restype = C.c_int
    if hasattr(L, "sgm_set_pixel_bits"):      # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_set_pixel_bits.argtypes = [C.c_void_p, C.c_int]
        L.sgm_set_pixel_bits.restype = C.c_bool
        L.SGM_SetPixelBits.argtypes = [C.c_int]
        L.SGM_SetPixelBits.restype = C.c_bool
    L.sgm_set_batch.argtypes = [C.c_void_p, C.c_int]
    L.sgm_set_batch.restype = C.c_bool
    L.sgm_select_frame.argtypes = [C.c_void_p, C.c_int]
    for f in (L.sgm_initialize, L.sgm_reset):
        f.argtypes = [C.c_void_p, C.c_uint16, C.c_uint16, opt_p]
        f.restype = C.c_bool
    for f in (L.sgm_match, L.sgm_match_device, L.sgm_match_async):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_bool
    L.sgm_match_wait.argtypes = [C.c_void_p]
    L.sgm_match_wait.restype = C.c_bool
    L.sgm_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.sgm_host_alloc.restype = C.c_void_p
    L.sgm_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.sgm_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_uint16, C.c_uint16, opt_p, C.c_void_p]
    L.sgm_compute.restype = C.c_bool
    L.sgm_synchronize.argtypes = [C.c_void_p]
    L.sgm_synchronize.restype = C.c_bool
    L.sgm_stream.argtypes = [C.c_void_p]
    L.sgm_stream.restype = C.c_void_p
    L.sgm_read_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.sgm_read_stage.restype = C.c_size_t
    L.sgm_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.sgm_set_rows.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.sgm_set_rows.restype = C.c_bool
    L.sgm_tile_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sgm_tile_begin.restype = C.c_bool
    L.sgm_tile_boundary_bytes.argtypes = [C.c_void_p]
    L.sgm_tile_boundary_bytes.restype = C.c_size_t
    for f in (L.sgm_tile_import_boundary, L.sgm_tile_export_boundary):
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        f.restype = C.c_bool
    L.sgm_tile_sweep.argtypes = [C.c_void_p, C.c_int]
    L.sgm_tile_sweep.restype = C.c_bool
    for f in (L.sgm_tile_finish, L.sgm_tile_post):
        f.argtypes = [C.c_void_p, C.c_void_p]
        f.restype = C.c_bool
    L.sgm_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.sgm_last_timing.restype = C.c_int
    L.sgm_mean_timing.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                  C.POINTER(C.c_long)]
    L.sgm_mean_timing.restype = C.c_int
    L.sgm_disparity_to_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.sgm_disparity_to_depth.restype = C.c_bool
    L.sgm_compare_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sgm_compare_depth.restype = C.c_bool
    L.sgm_gray_from_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.sgm_gray_from_planes.restype = C.c_bool
    for name in ("sgm_match_planes_async", "sgm_match_planes"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]
        getattr(L, name).restype = C.c_bool
    L.sgm_host_walk_line.argtypes = [C.c_int] * 5 + [C.c_void_p]
    L.sgm_host_walk_line.restype = C.c_int
    L.sgm_host_anomalous_line.argtypes = [C.c_int, C.c_int]
    L.sgm_host_anomalous_line.restype = C.c_int
    L.sgm_host_p2_table.argtypes = [C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "sgm_debug_guard_check"):   # (SGM_LIBRARY_PATH may point an A/B run at a build of older sources)
        L.sgm_debug_guard_check.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.sgm_debug_guard_check.restype = C.c_int
    return L


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64/libhsa; a
    second runtime (the system one libsgm_mi355x.so is linked against) initialised in the same
    process finds no GPU.  Python callers use torch for device memory and torch.distributed, so
    before loading our library we promote torch's already-loaded runtime to the global symbol
    scope: the HIP calls and the kernel registration of libsgm_mi355x.so then bind to it.  A plain C
    caller (no torch in the process) simply gets the system runtime the library is linked to."""
    try:
        import torch  # noqa: F401
    except Exception:
        return
    bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)


def synth_pair(width, height, disparity_range, seed):
    """Seeded synthetic stereo pair from the library's own host generator."""
    L = load_library()
    left = np.empty((height, width), np.uint8)
    right = np.empty((height, width), np.uint8)
    L.SGM_SynthPair(width, height, disparity_range, seed & 0xFFFFFFFF, left.ctypes.data, right.ctypes.data)
    return left, right


def debug_guard_check():
    """sgm_debug_guard_check: (violated bands, live allocations, live bytes) of the debug allocation mode (SGM_DEBUG_GUARD /
    SGM_DEBUG_POISON in the environment when the buffers were allocated; include/sgm_mi355x.h).  (0, 0, 0) with the mode off."""
    live, size = C.c_int(0), C.c_size_t(0)
    bad = load_library().sgm_debug_guard_check(C.byref(live), C.byref(size))
    return int(bad), int(live.value), int(size.value)


def set_refine(enable=True, lam=REFINE_LAMBDA, sigma=REFINE_SIGMA, iterations=REFINE_ITERS, keep_invalid=False) -> bool:
    """SGM_SetRefine: the refinement of the default instance (SGM_Initialize / SGM_Reset / SGM_Match); include/sgm_mi355x.h has the
    contract.  Takes effect at the next initialize / reset; False for parameters out of range."""
    return bool(load_library().SGM_SetRefine(int(enable), lam, sigma, int(iterations), int(keep_invalid)))


def refine_table(lam, sigma, iterations, t):
    """sgm_refine_table: the float32 weight table L_t[256] of iteration t (host only)."""
    out = np.zeros(256, np.float32)
    if not load_library().sgm_refine_table(lam, sigma, int(iterations), int(t), out.ctypes.data):
        raise ValueError(f"sgm_refine_table: arguments out of range ({lam}, {sigma}, {iterations}, {t})")
    return out


def rectify_maps(K, dist, R, Knew, width, height):
    """sgm_rectify_maps: (map_x, map_y), float32 [height][width] each, of one camera by the formulas of OpenCV's
    initUndistortRectifyMap (host only).  K, R, Knew: 3x3; dist: k1 k2 p1 p2 k3."""
    mats = [np.ascontiguousarray(m, np.float64).reshape(-1) for m in (K, dist, R, Knew)]
    if [m.size for m in mats] != [9, 5, 9, 9]:
        raise ValueError("rectify_maps: K, R, Knew are 3x3, dist has 5 coefficients")
    map_x = np.empty((int(height), int(width)), np.float32)
    map_y = np.empty((int(height), int(width)), np.float32)
    if not load_library().sgm_rectify_maps(*(m.ctypes.data for m in mats), int(width), int(height), map_x.ctypes.data,
                                           map_y.ctypes.data):
        raise ValueError("sgm_rectify_maps: a size below 1 or a singular Knew R")
    return map_x, map_y


def rectify_valid_mask(map_x, map_y):
    """sgm_rectify_valid_mask: uint8 [H][W], 1 where all four taps of SGM_SetRectify's sampling of that output pixel fall inside
    the source image (host only; one camera's maps)."""
    mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    if mx.ndim != 2 or mx.shape != my.shape:
        raise ValueError("rectify_valid_mask: two float32 maps of one shape [H][W] are needed")
    h, w = mx.shape
    mask = np.empty((h, w), np.uint8)
    if not load_library().sgm_rectify_valid_mask(w, h, mx.ctypes.data, my.ctypes.data, mask.ctypes.data):
        raise ValueError("sgm_rectify_valid_mask: a size below 1")
    return mask


def _read_cloud(call, spec):
    """(points, offsets) through a sgm_read_cloud-shaped call(spec, points, capacity, offsets): sized from a first call that copies
    the offsets alone; None where the C call refuses the spec."""
    offsets = np.zeros(max(int(spec.frames), 0) + 1, np.uint32)
    if call(C.byref(spec), None, 0, offsets.ctypes.data):
        return np.empty(0, POINT_DTYPE), offsets                  # an empty cloud
    total = int(offsets[-1])
    if total == 0:
        return None
    points = np.empty(total, POINT_DTYPE)
    if not call(C.byref(spec), points.ctypes.data, total, offsets.ctypes.data):
        return None
    return points, offsets


def _temporal_stats(call, maps):
    """uint32 [maps][5] through a sgm_temporal_stats-shaped call(out, capacity); None where it returns no entries"""
    out = np.zeros((max(int(maps), 1), 5), np.uint32)
    n = call(out.ctypes.data, out.shape[0])
    return out[:n] if n > 0 else None


def _rectify_args(maps):
    """(width, height, four pointers, the arrays kept alive) for sgm_set_rectify / SGM_SetRectify; None first = off"""
    if maps[0] is None:
        return 0, 0, [None] * 4, []
    arrays = [np.ascontiguousarray(m, np.float32) for m in maps]
    if arrays[0].ndim != 2 or any(a.shape != arrays[0].shape for a in arrays):
        raise ValueError("set_rectify: four float32 maps of one shape [H][W] are needed")
    h, w = arrays[0].shape
    return w, h, [a.ctypes.data for a in arrays], arrays


def _device_ptr(x, dtype, count, name):
    """A device pointer from an int or a torch tensor (checked: contiguous, dtype, number of elements)."""
    if isinstance(x, int):
        return x
    import torch
    want = {np.float32: torch.float32, np.uint16: torch.uint16 if hasattr(torch, "uint16") else torch.int16,
            np.uint8: torch.uint8}[dtype]
    ok_dtype = x.dtype == want or (dtype is np.uint16 and x.dtype in (torch.int16,))
    if not (x.is_cuda and x.is_contiguous() and ok_dtype and x.numel() == count):
        raise ValueError(f"{name}: a contiguous device tensor of {count} {np.dtype(dtype).name} elements is needed")
    return x.data_ptr()


def _pixel_dtype(bits):
    return np.uint16 if bits > 8 else np.uint8


class _StageReader:
    _wide_window, _census_kind = False, CENSUS_CENTRE
    _bits_req = _bits = 8            # bits per sample asked for (set_pixel_bits) / in effect since the last initialize or reset

    def _img(self, a, bits=None):
        """A C-contiguous image of the dtype the instance reads: uint8, or uint16 with more than 8 bits per sample in effect
        (bits: another width than the one in effect).  The C side moves width * height samples of that size whatever the array
        holds, so any other dtype is a TypeError."""
        a = np.ascontiguousarray(a)
        bits = self._bits if bits is None else bits
        want = _pixel_dtype(bits)
        if a.dtype != want:
            raise TypeError(f"images must be {np.dtype(want).name} with {bits} bits per sample (set_pixel_bits), got {a.dtype}")
        return a

    @property
    def wide_census(self):
        """u64 census words and a materialised cost volume: a window other than 5x5 with the centre census.  The symmetric
        kind has u32 words for any window."""
        return self._wide_window and self._census_kind == CENSUS_CENTRE

    def _read(self, which):
        raise NotImplementedError

    def read_stage(self, which):
        """Copy one intermediate buffer of the last match to the host (parity tests)."""
        idx = STAGE_NAMES.index(which) if isinstance(which, str) else which
        h, w, d = self.shape
        if idx < 2 and self.wide_census:
            dt, shp = np.uint64, (h, w)
        elif idx == STAGE_FILLED:
            dt, shp = np.float32, (h, w)
        elif idx in (STAGE_RECT_LEFT, STAGE_RECT_RIGHT):
            dt, shp = _pixel_dtype(self._bits), (h, w)
        elif idx in (STAGE_FILL_CLASS, STAGE_NARROW_LEFT, STAGE_NARROW_RIGHT):
            dt, shp = np.uint8, (h, w)
        elif idx in (STAGE_RIGHT_AFTER_LR, STAGE_RIGHT_AFTER_SPECKLE, STAGE_RIGHT_FINAL, STAGE_TEMPORAL_IN, STAGE_TEMPORAL_VALUE,
                     STAGE_RIGHT_TEMPORAL_IN, STAGE_RIGHT_TEMPORAL_VALUE):
            dt, shp = np.float32, (h, w)
        elif idx in (STAGE_TEMPORAL_BITS, STAGE_RIGHT_TEMPORAL_BITS):
            dt, shp = np.uint8, (h, w)
        elif idx >= 10:
            dt, shp = np.uint8, (h, w, d)
        else:
            dt, shp = _STAGE_DTYPE[idx], ((h, w, d) if idx in (2, 3) else (h, w))
        out = np.empty(shp, dt)
        got = self._read(idx, out)
        if got != out.nbytes:
            raise RuntimeError(f"read_stage({which}) returned {got} of {out.nbytes} bytes")
        return out

    def read_stages(self):
        return {n: self.read_stage(n) for n in STAGE_NAMES}

    def read_filled(self):
        """Stage 9: the map after hole filling, before the median (needs keep_stages and fill on)."""
        return self.read_stage(STAGE_FILLED)

    def read_rectified(self):
        """Stages 19 and 20: the rectified (left, right) images the last match ran on (needs rectification on, set_rectify)."""
        return self.read_stage(STAGE_RECT_LEFT), self.read_stage(STAGE_RECT_RIGHT)

    def read_narrowed(self):
        """Stages 21 and 22: the narrowed (left, right) images g8 = min(v >> (bits - 8), 255) of the last match (needs more than 8
        bits per sample in effect, set_pixel_bits)."""
        return self.read_stage(STAGE_NARROW_LEFT), self.read_stage(STAGE_NARROW_RIGHT)

    def read_temporal(self, right=False):
        """Stages 30 and 31 (33 and 34 with right, after a match_both): the temporal filter's history (hv float32, hb uint8) of the
        selected frame's stream after the last match (needs set_temporal in effect)."""
        if right:
            return self.read_stage(STAGE_RIGHT_TEMPORAL_VALUE), self.read_stage(STAGE_RIGHT_TEMPORAL_BITS)
        return self.read_stage(STAGE_TEMPORAL_VALUE), self.read_stage(STAGE_TEMPORAL_BITS)

    def read_fill_classes(self):
        """Stage 18: the hole-filling classes, 0 valid / 1 occluded / 2 mismatched (after any match with fill on)."""
        return self.read_stage(STAGE_FILL_CLASS)


class SGM(_StageReader):
    """The reference's global-instance API: SGM_Initialize / SGM_Reset / SGM_Match.  The default instance is one per process in C,
    and so are its bits per sample: every SGM object reads and writes them on the class (SGM._bits_req / SGM._bits), so that a
    second object, or one made after set_pixel_bits, checks image dtypes against the width the library really reads."""

    def __init__(self):
        self.lib = load_library()
        self.shape = None

    def set_device(self, ordinal) -> bool:
        return bool(self.lib.SGM_SetDevice(ordinal))

    def set_honor_num_paths(self, honor):
        self.lib.SGM_SetHonorNumPaths(int(honor))

    def set_census_window(self, width: int, height: int) -> bool:
        ok = bool(self.lib.SGM_SetCensusWindow(width, height))
        if ok:
            self._wide_window = not (width == 5 and height == 5)
        return ok

    def set_census_kind(self, kind: int) -> bool:
        """Extension: CENSUS_CENTRE (reference) or CENSUS_SYMMETRIC, the centre-symmetric census on the fast path for any window
        (include/sgm_mi355x.h, SGM_SetCensusKind); next initialize/reset."""
        ok = bool(self.lib.SGM_SetCensusKind(int(kind)))
        if ok:
            self._census_kind = int(kind)
        return ok

    def set_reference_view(self, right: bool):
        self.lib.SGM_SetReferenceView(int(right))

    def set_pixel_bits(self, bits: int) -> bool:
        """Extension: bits per image sample, 8 (reference) or 9..16: from the next initialize/reset on the images of every match
        are uint16 arrays (include/sgm_mi355x.h, SGM_SetPixelBits).  False, and nothing changes, for any other value."""
        ok = bool(self.lib.SGM_SetPixelBits(int(bits)))
        if ok:
            SGM._bits_req = int(bits)
        return ok

    def set_fill_holes(self, enable: bool = True) -> bool:
        """Extension: occlusion-aware hole filling of the +INF pixels (include/sgm_mi355x.h); next initialize/reset."""
        return bool(self.lib.SGM_SetFillHoles(int(enable)))

    def set_refine(self, enable=True, lam=REFINE_LAMBDA, sigma=REFINE_SIGMA, iterations=REFINE_ITERS, keep_invalid=False) -> bool:
        """Extension: confidence-guided edge-aware refinement of the map (include/sgm_mi355x.h); next initialize/reset."""
        return set_refine(enable, lam, sigma, iterations, keep_invalid)

    def set_rectify(self, map_lx, map_ly=None, map_rx=None, map_ry=None) -> bool:
        """Extension: rectify raw camera pairs on the device ahead of every match, through OpenCV-style float32 maps [H][W] of
        the left and the right camera (include/sgm_mi355x.h, SGM_SetRectify); None turns it off; next initialize/reset."""
        w, h, ptrs, _keep = _rectify_args((map_lx, map_ly, map_rx, map_ry))
        return bool(self.lib.SGM_SetRectify(w, h, *ptrs))

    def set_temporal(self, spec) -> bool:
        """Extension: the temporal filter of a stream of matches (include/sgm_mi355x.h, sgm_temporal_spec); None turns it off; next
        initialize/reset.  The history survives the per-frame reset.  False for a spec out of range."""
        return bool(self.lib.SGM_SetTemporal(C.byref(spec) if spec is not None else None))

    def temporal_restart(self) -> bool:
        """SGM_TemporalRestart: the next filtered match starts from an empty history (a scene cut)."""
        return bool(self.lib.SGM_TemporalRestart())

    def temporal_stats(self):
        """SGM_TemporalStats: uint32 [1][5], the decisions of the last match per class (TEMPORAL_CLASSES), or None when the spec's
        stats is off."""
        return _temporal_stats(self.lib.SGM_TemporalStats, 1)

    def keep_stages(self, enable=True):
        self.lib.SGM_KeepStages(int(enable))

    def initialize(self, width, height, option) -> bool:
        ok = bool(self.lib.SGM_Initialize(width, height, C.byref(option)))
        if ok:
            SGM._bits = SGM._bits_req
            self.shape = (height, width, option.max_disparity - option.min_disparity)
        return ok

    def reset(self, width, height, option) -> bool:
        ok = bool(self.lib.SGM_Reset(width, height, C.byref(option)))
        if ok:
            SGM._bits = SGM._bits_req
            self.shape = (height, width, option.max_disparity - option.min_disparity)
        return ok

    def match(self, left, right):
        """Returns the float32 disparity map, or None where the C call returns false."""
        if left is None or right is None:
            assert not self.lib.SGM_Match(None, None, None)
            return None
        left, right = self._img(left), self._img(right)
        out = np.empty(left.shape, np.float32)
        ok = self.lib.SGM_Match(left.ctypes.data, right.ctypes.data, out.ctypes.data)
        return out if ok else None

    def match_confidence(self, left, right):
        """SGM_MatchConfidence: (disparity float32, confidence uint16) of the default instance, or None where the C call returns
        false.  The confidence contract is in include/sgm_mi355x.h."""
        left, right = self._img(left), self._img(right)
        out = np.empty(left.shape, np.float32)
        conf = np.empty(left.shape, np.uint16)
        ok = self.lib.SGM_MatchConfidence(left.ctypes.data, right.ctypes.data, out.ctypes.data, conf.ctypes.data)
        return (out, conf) if ok else None

    def match_both(self, left, right):
        """SGM_MatchBoth: (left-view map, right-view map) of the default instance from one match, float32 each, or None where the C
        call returns false.  The contract is in include/sgm_mi355x.h."""
        left, right = self._img(left), self._img(right)
        out_l = np.empty(left.shape, np.float32)
        out_r = np.empty(left.shape, np.float32)
        ok = self.lib.SGM_MatchBoth(left.ctypes.data, right.ctypes.data, out_l.ctypes.data, out_r.ctypes.data)
        return (out_l, out_r) if ok else None

    def compute(self, left, right, option, out=None):
        """sgm_compute: SGM_Reset + SGM_Match in one call (north_star's entry point).  None where it returns false.  `out`: a
        C-contiguous float32 [H][W] array to write into (a caller with a stream of frames allocates it once)."""
        left, right = self._img(left, SGM._bits_req), self._img(right, SGM._bits_req)    # the call resets first: the bits asked for hold
        h, w = left.shape
        if out is None:
            out = np.empty((h, w), np.float32)
        elif out.dtype != np.float32 or tuple(out.shape) != (h, w) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"compute: out must be a C-contiguous float32 array of shape {(h, w)}")
        ok = self.lib.sgm_compute(left.ctypes.data, right.ctypes.data, w, h, C.byref(option), out.ctypes.data)
        if ok:
            SGM._bits = SGM._bits_req
            self.shape = (h, w, option.max_disparity - option.min_disparity)
        return out if ok else None

    def match_device(self, d_left: int, d_right: int, d_out: int) -> bool:
        return bool(self.lib.SGM_MatchDevice(d_left, d_right, d_out))

    def synchronize(self) -> bool:
        return bool(self.lib.SGM_Synchronize())

    def read_cloud(self, spec: SGMCloudSpec):
        """SGM_ReadCloud: (points as POINT_DTYPE records, offsets uint32 [frames + 1]) of the last match's final map, or None
        where the C call returns false.  The contract is in include/sgm_mi355x.h (sgm_cloud_spec)."""
        return _read_cloud(self.lib.SGM_ReadCloud, spec)

    def match_scaled(self, spec: SGMScaleSpec, left, right):
        """SGM_MatchScaled: one FULL-resolution pair through the default instance, initialised at the low-resolution shape; the
        full-resolution float32 map, or None where the C call returns false (include/sgm_mi355x.h, sgm_scale_spec)."""
        left, right = self._img(left, spec.bits), self._img(right, spec.bits)
        want = (spec.height, spec.width)
        if tuple(left.shape) != want or tuple(right.shape) != want:
            raise ValueError(f"expected images of shape {want}, got {left.shape} and {right.shape}")
        out = np.empty(want, np.float32)
        ok = self.lib.SGM_MatchScaled(C.byref(spec), left.ctypes.data, right.ctypes.data, out.ctypes.data)
        return out if ok else None

    def shutdown(self):
        self.lib.SGM_Shutdown()

    def _read(self, idx, out):
        return self.lib.SGM_ReadStage(idx, out.ctypes.data, out.nbytes)


class SGMInstance(_StageReader):
    """Explicit instance (extension): own HIP stream and buffers on one GPU."""

    def __init__(self, device=0, batch=1):
        self.lib = load_library()
        self.handle = self.lib.sgm_create(device)
        if not self.handle:
            raise RuntimeError(f"sgm_create({device}) failed: no usable gfx950 device (no CPU fallback)")
        self.device = device
        self.shape = None
        self.batch = 1
        self._pinned = []
        if batch != 1:
            self.set_batch(batch)

    def set_batch(self, frames: int) -> bool:
        """Frames per match call ([frames][H][W] arrays); takes effect at the next initialize/reset."""
        ok = bool(self.lib.sgm_set_batch(self.handle, frames))
        if ok:
            self.batch = frames
        return ok

    def select_frame(self, frame: int):
        """Which frame of the batch read_stage() returns."""
        self.lib.sgm_select_frame(self.handle, frame)

    def close(self):
        if self.handle:
            self.lib.sgm_match_wait(self.handle)
            for p in self._pinned:
                self.lib.sgm_host_free(self.handle, p)
            self._pinned = []
            self.lib.sgm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_honor_num_paths(self, honor):
        self.lib.sgm_set_honor_num_paths(self.handle, int(honor))

    def set_overlap_post(self, enable: bool = True) -> bool:
        """The post pass (LR check, speckle, median) of a match on a second stream beside the next match's aggregation;
        results are complete after synchronize(), not in order of `stream` (include/sgm_mi355x.h)."""
        return bool(self.lib.sgm_set_overlap_post(self.handle, int(enable)))

    STAGE_MAIN, STAGE_SUM, STAGE_POST = 0, 1, 2

    def set_stage_cus(self, which: int, first_cu_per_xcd: int = 0, cus_per_xcd: int = 0) -> bool:
        """sgm_set_stage_cus: stage group `which` (STAGE_MAIN census + aggregation, STAGE_SUM cost sum + WTAs, STAGE_POST LR check +
        speckle + median) on a stream of its own restricted to CUs [first, first + count) of every XCD (count 0: all CUs,
        count < 0: back to the default)."""
        return bool(self.lib.sgm_set_stage_cus(self.handle, which, first_cu_per_xcd, cus_per_xcd))

    def set_cu_split(self, spec: str) -> bool:
        """'post=0:2,sum=2:8,main=10:22' -> set_stage_cus per group ('first:count' CUs per XCD; 'post' alone = 'post=0:0')."""
        which = {"main": self.STAGE_MAIN, "sum": self.STAGE_SUM, "post": self.STAGE_POST}
        ok = True
        for item in filter(None, (t.strip() for t in spec.split(","))):
            name, _, rng = item.partition("=")
            if rng.startswith("p"):                           # 'sum=p-1': own stream with dispatch priority -1 (higher)
                ok = bool(self.lib.sgm_set_stage_priority(self.handle, which[name], int(rng[1:]))) and ok
                continue
            first, _, count = (rng or "0:0").partition(":")
            ok = self.set_stage_cus(which[name], int(first or 0), int(count or 0)) and ok
        return ok

    def set_census_window(self, width: int, height: int) -> bool:
        """Extension: odd census window of at most 64 pixels (5x5 = reference); next initialize/reset."""
        ok = bool(self.lib.sgm_set_census_window(self.handle, width, height))
        if ok:
            self._wide_window = not (width == 5 and height == 5)
        return ok

    def set_census_kind(self, kind: int) -> bool:
        """Extension: CENSUS_CENTRE (reference) or CENSUS_SYMMETRIC, the centre-symmetric census on the fast path for any window
        (include/sgm_mi355x.h, SGM_SetCensusKind); next initialize/reset."""
        ok = bool(self.lib.sgm_set_census_kind(self.handle, int(kind)))
        if ok:
            self._census_kind = int(kind)
        return ok

    def set_reference_view(self, right: bool):
        """Extension: True = the result is the right image's disparity map (mirrored LR check)."""
        self.lib.sgm_set_reference_view(self.handle, int(right))

    def set_pixel_bits(self, bits: int) -> bool:
        """Extension: bits per image sample, 8 (reference) or 9..16: from the next initialize/reset on the images of every match
        are uint16 arrays (device images: uint16, 2-byte aligned) (include/sgm_mi355x.h, SGM_SetPixelBits).  False, and nothing
        changes, for any other value."""
        ok = bool(self.lib.sgm_set_pixel_bits(self.handle, int(bits)))
        if ok:
            self._bits_req = int(bits)
        return ok

    def set_fill_holes(self, enable: bool = True) -> bool:
        """Extension: occlusion-aware hole filling of the +INF pixels (include/sgm_mi355x.h); next initialize/reset."""
        return bool(self.lib.sgm_set_fill_holes(self.handle, int(enable)))

    def fill_holes(self, d_disp: int, d_class: int = None) -> bool:
        """sgm_fill_holes: fill the +INF pixels of a device map of the instance's batch and shape in place (passes 1 and 2 need
        the u8 class map d_class, None runs pass 3 alone); asynchronous on `stream`."""
        return bool(self.lib.sgm_fill_holes(self.handle, d_disp, d_class or None))

    def set_refine(self, enable=True, lam=REFINE_LAMBDA, sigma=REFINE_SIGMA, iterations=REFINE_ITERS, keep_invalid=False) -> bool:
        """Extension: confidence-guided edge-aware refinement of the map (include/sgm_mi355x.h); next initialize/reset.  False for
        parameters out of range."""
        return bool(self.lib.sgm_set_refine(self.handle, int(enable), lam, sigma, int(iterations), int(keep_invalid)))

    def set_rectify(self, map_lx, map_ly=None, map_rx=None, map_ry=None) -> bool:
        """Extension: rectify raw camera pairs on the device ahead of every match, through OpenCV-style float32 maps [H][W] of
        the left and the right camera (include/sgm_mi355x.h, SGM_SetRectify); None turns it off; next initialize/reset."""
        w, h, ptrs, _keep = _rectify_args((map_lx, map_ly, map_rx, map_ry))
        return bool(self.lib.sgm_set_rectify(self.handle, w, h, *ptrs))

    def set_temporal(self, spec) -> bool:
        """Extension: the temporal filter of a stream of matches (include/sgm_mi355x.h, sgm_temporal_spec); None turns it off; next
        initialize/reset.  One instance is one stream per frame of its batch (spec.sequence = 0) or one stream whose consecutive
        frames are the frames of a batch (1); the history survives the per-frame reset.  False for a spec out of range."""
        return bool(self.lib.sgm_set_temporal(self.handle, C.byref(spec) if spec is not None else None))

    def temporal_restart(self) -> bool:
        """sgm_temporal_restart: the next filtered match starts from an empty history (a scene cut)."""
        return bool(self.lib.sgm_temporal_restart(self.handle))

    def temporal_stats(self):
        """sgm_temporal_stats: uint32 [batch * views][5], the decisions of the last match per map and class (TEMPORAL_CLASSES);
        None when the spec's stats is off or nothing was filtered.  Blocking."""
        return _temporal_stats(lambda *a: self.lib.sgm_temporal_stats(self.handle, *a), 2 * self.batch)

    def temporal_filter(self, spec, streams: int, steps: int, pixels: int, d_maps: int, d_conf, d_hist_value: int, d_hist_bits: int,
                        d_stats=None) -> bool:
        """sgm_temporal_filter: the filter on any device maps float32 [streams][steps][pixels], in place, with the caller's history
        (float32 / uint8 [streams][pixels]); d_conf (uint16) / d_stats (uint32 [streams * steps][5]) None: none.  Device pointers;
        asynchronous on `stream`."""
        return bool(self.lib.sgm_temporal_filter(self.handle, C.byref(spec), streams, steps, pixels, d_maps, d_conf or None,
                                                 d_hist_value, d_hist_bits, d_stats or None))

    def temporal_clear(self, streams: int, pixels: int, d_hist_value: int, d_hist_bits: int) -> bool:
        """sgm_temporal_clear: +INF / 0 into a history of streams x pixels entries; asynchronous on `stream`."""
        return bool(self.lib.sgm_temporal_clear(self.handle, streams, pixels, d_hist_value, d_hist_bits))

    def rectify(self, d_left, d_right, d_out_left, d_out_right) -> bool:
        """sgm_rectify: the remap alone on device images of the instance's batch and shape (uint8, or uint16 with more than 8 bits
        per sample in effect; device pointers or torch tensors), through the maps in effect; asynchronous on `stream`.  False when no maps are in effect."""
        n = self.batch * self.shape[0] * self.shape[1] if self.shape else 0
        return bool(self.lib.sgm_rectify(self.handle, *(_device_ptr(x, _pixel_dtype(self._bits), n, name) for x, name in
                                                        ((d_left, "d_left"), (d_right, "d_right"), (d_out_left, "d_out_left"),
                                                         (d_out_right, "d_out_right")))))

    def refine_disparity(self, d_disp, d_conf, d_guide) -> bool:
        """sgm_refine_disparity: refine a device map of the instance's batch and shape in place with the parameters of the last
        set_refine(True, ...), from the confidence (uint16) and the grey image (uint8); device pointers or torch tensors.
        Asynchronous on `stream`."""
        n = self.batch * self.shape[0] * self.shape[1] if self.shape else 0
        return bool(self.lib.sgm_refine_disparity(self.handle, _device_ptr(d_disp, np.float32, n, "d_disp"),
                                                  _device_ptr(d_conf, np.uint16, n, "d_conf"),
                                                  _device_ptr(d_guide, np.uint8, n, "d_guide")))

    def keep_stages(self, enable=True):
        self.lib.sgm_keep_stages(self.handle, int(enable))

    def fused_sweep_rows(self) -> int:
        """Rows per workgroup of the fused last sweep in the LAST match, 0 if it ran the separate kernels."""
        self.lib.sgm_fused_sweep_rows.argtypes = [C.c_void_p]
        self.lib.sgm_fused_sweep_rows.restype = C.c_int
        return int(self.lib.sgm_fused_sweep_rows(self.handle))

    def enable_timing(self, enable=True):
        self.lib.sgm_enable_timing(self.handle, int(enable))

    def last_timing(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = self.lib.sgm_last_timing(self.handle, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    def mean_timing(self):
        """({stage: mean ms}, {stage: min ms}, matches) over every match since enable_timing()."""
        names = (C.c_char_p * 16)()
        mean = (C.c_float * 16)()
        mn = (C.c_float * 16)()
        cnt = C.c_long(0)
        n = self.lib.sgm_mean_timing(self.handle, names, mean, mn, 16, C.byref(cnt))
        return ({names[i].decode(): float(mean[i]) for i in range(n)},
                {names[i].decode(): float(mn[i]) for i in range(n)}, int(cnt.value))

    def initialize(self, width, height, option) -> bool:
        ok = bool(self.lib.sgm_initialize(self.handle, width, height, C.byref(option)))
        if ok:
            self._bits = self._bits_req
            self.shape = (height, width, option.max_disparity - option.min_disparity)
        return ok

    def reset(self, width, height, option) -> bool:
        ok = bool(self.lib.sgm_reset(self.handle, width, height, C.byref(option)))
        if ok:
            self._bits = self._bits_req
            self.shape = (height, width, option.max_disparity - option.min_disparity)
        return ok

    def match(self, left, right):
        """left/right: uint8 (uint16 with more than 8 bits per sample in effect, set_pixel_bits) [H][W], or [batch][H][W] when the
        instance has a batch > 1."""
        if self.shape is None:
            return None                                   # Match before Initialize: false in the reference (.c:70)
        left, right = self._img(left), self._img(right)
        want = self.shape[:2] if self.batch == 1 else (self.batch,) + tuple(self.shape[:2])
        if tuple(left.shape) != tuple(want):
            raise ValueError(f"expected images of shape {want}, got {left.shape}")
        out = np.empty(left.shape, np.float32)
        ok = self.lib.sgm_match(self.handle, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        return out if ok else None

    def match_async(self, left, right, out) -> bool:
        """sgm_match_async: queue upload + pipeline + download and return.  `left`, `right` (uint8) and `out` (float32)
        must be C-contiguous arrays of the instance's shape that stay alive and untouched until match_wait()."""
        if self.shape is None:
            return False                                  # Match before Initialize: false in the reference (.c:70)
        for a in (left, right, out):
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError("match_async needs C-contiguous arrays")
        px = _pixel_dtype(self._bits)
        if left.dtype != px or right.dtype != px or out.dtype != np.float32:
            raise TypeError(f"match_async: {np.dtype(px).name} images ({self._bits} bits per sample), float32 output")
        # the C side moves batch * W * H bytes (4x that for the output) whatever the arrays hold: check before handing pointers over
        want = self._frame_shape()
        for name, a in (("left", left), ("right", right), ("out", out)):
            if tuple(a.shape) != want:
                raise ValueError(f"match_async: {name} has shape {tuple(a.shape)}, the instance expects {want}")
        return bool(self.lib.sgm_match_async(self.handle, left.ctypes.data, right.ctypes.data, out.ctypes.data))

    def match_confidence(self, left, right):
        """sgm_match_confidence: (disparity float32, confidence uint16), each of the instance's shape, or None where the C call
        returns false.  The confidence contract is in include/sgm_mi355x.h."""
        if self.shape is None:
            return None
        left, right = self._img(left), self._img(right)
        want = self._frame_shape()
        if tuple(left.shape) != want or tuple(right.shape) != want:
            raise ValueError(f"expected images of shape {want}, got {left.shape}")
        out = np.empty(want, np.float32)
        conf = np.empty(want, np.uint16)
        ok = self.lib.sgm_match_confidence(self.handle, left.ctypes.data, right.ctypes.data, out.ctypes.data, conf.ctypes.data)
        return (out, conf) if ok else None

    def match_confidence_async(self, left, right, out, conf) -> bool:
        """sgm_match_confidence_async: as match_async, plus `conf` (uint16, the instance's shape) which stays borrowed until
        match_wait() as well."""
        if self.shape is None:
            return False
        want = self._frame_shape()
        px = _pixel_dtype(self._bits)
        for name, a, dt in (("left", left, px), ("right", right, px), ("out", out, np.float32), ("conf", conf, np.uint16)):
            if a.dtype != dt and name in ("left", "right"):
                raise TypeError(f"match_confidence_async: {name} must be {np.dtype(dt).name} with {self._bits} bits per sample")
            if not a.flags["C_CONTIGUOUS"] or a.dtype != dt or tuple(a.shape) != want:
                raise ValueError(f"match_confidence_async: {name} must be a C-contiguous {np.dtype(dt).name} array of shape {want}")
        return bool(self.lib.sgm_match_confidence_async(self.handle, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                        conf.ctypes.data))

    def match_confidence_device(self, d_left: int, d_right: int, d_out: int, d_conf: int) -> bool:
        """sgm_match_confidence_device: device pointers (d_conf: uint16 [batch][H][W]); asynchronous on the instance stream."""
        return bool(self.lib.sgm_match_confidence_device(self.handle, d_left, d_right, d_out, d_conf))

    def match_both(self, left, right):
        """sgm_match_both: (left-view map, right-view map) from one match, float32 of the instance's shape each, or None where the
        C call returns false.  The contract is in include/sgm_mi355x.h (SGM_MatchBoth)."""
        if self.shape is None:
            return None
        left, right = self._img(left), self._img(right)
        want = self._frame_shape()
        if tuple(left.shape) != want or tuple(right.shape) != want:
            raise ValueError(f"expected images of shape {want}, got {left.shape}")
        out_l = np.empty(want, np.float32)
        out_r = np.empty(want, np.float32)
        ok = self.lib.sgm_match_both(self.handle, left.ctypes.data, right.ctypes.data, out_l.ctypes.data, out_r.ctypes.data)
        return (out_l, out_r) if ok else None

    def match_both_async(self, left, right, out_left, out_right) -> bool:
        """sgm_match_both_async: as match_async with two float32 outputs; all four arrays stay borrowed until match_wait()."""
        if self.shape is None:
            return False
        want = self._frame_shape()
        px = _pixel_dtype(self._bits)
        for name, a, dt in (("left", left, px), ("right", right, px), ("out_left", out_left, np.float32),
                            ("out_right", out_right, np.float32)):
            if a.dtype != dt and name in ("left", "right"):
                raise TypeError(f"match_both_async: {name} must be {np.dtype(dt).name} with {self._bits} bits per sample")
            if not a.flags["C_CONTIGUOUS"] or a.dtype != dt or tuple(a.shape) != want:
                raise ValueError(f"match_both_async: {name} must be a C-contiguous {np.dtype(dt).name} array of shape {want}")
        return bool(self.lib.sgm_match_both_async(self.handle, left.ctypes.data, right.ctypes.data, out_left.ctypes.data,
                                                  out_right.ctypes.data))

    def match_both_device(self, d_left: int, d_right: int, d_out_left: int, d_out_right: int) -> bool:
        """sgm_match_both_device: device pointers (two float32 [batch][H][W] outputs); asynchronous on the instance stream."""
        return bool(self.lib.sgm_match_both_device(self.handle, d_left, d_right, d_out_left, d_out_right))

    def _frame_shape(self):
        h, w = self.shape[:2]
        return (h, w) if self.batch == 1 else (self.batch, h, w)

    def match_wait(self) -> bool:
        return bool(self.lib.sgm_match_wait(self.handle))

    def host_array(self, shape, dtype):
        """A numpy array in page-locked host memory (sgm_host_alloc): sgm_match_async uses it in place, without the
        staging copy.  Freed when the instance is closed; do not use it after that."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.sgm_host_alloc(self.handle, n)
        if not p:
            raise MemoryError("sgm_host_alloc failed")
        self._pinned.append(p)
        buf = (C.c_uint8 * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def match_device(self, d_left: int, d_right: int, d_out: int) -> bool:
        """Device pointers (e.g. torch tensor .data_ptr()); asynchronous on the instance stream."""
        return bool(self.lib.sgm_match_device(self.handle, d_left, d_right, d_out))

    def synchronize(self) -> bool:
        return bool(self.lib.sgm_synchronize(self.handle))

    # ---- row tiles (one frame over several GPUs; include/sgm_mi355x.h "row tiles"); all device pointers ----
    def set_rows(self, row_begin: int, row_end: int) -> bool:
        """This instance computes rows [row_begin, row_end) from the next initialize/reset on; (0, 0) = whole frames."""
        return bool(self.lib.sgm_set_rows(self.handle, row_begin, row_end))

    def tile_begin(self, d_left: int, d_right: int) -> bool:
        return bool(self.lib.sgm_tile_begin(self.handle, d_left, d_right))

    def tile_boundary_bytes(self) -> int:
        return int(self.lib.sgm_tile_boundary_bytes(self.handle))

    def tile_import_boundary(self, forward: bool, d_buf: int) -> bool:
        return bool(self.lib.sgm_tile_import_boundary(self.handle, int(forward), d_buf))

    def tile_sweep(self, forward: bool) -> bool:
        return bool(self.lib.sgm_tile_sweep(self.handle, int(forward)))

    def tile_export_boundary(self, forward: bool, d_buf: int) -> bool:
        return bool(self.lib.sgm_tile_export_boundary(self.handle, int(forward), d_buf))

    def tile_finish(self, d_disp: int) -> bool:
        return bool(self.lib.sgm_tile_finish(self.handle, d_disp))

    def tile_post(self, d_disp: int) -> bool:
        return bool(self.lib.sgm_tile_post(self.handle, d_disp))

    # ---- test-platform arithmetic on device buffers (include/sgm_mi355x.h) ----
    def disparity_to_depth(self, d_disp: int, count: int, fx: float, baseline: float, doffs: float, d_depth: int) -> bool:
        return bool(self.lib.sgm_disparity_to_depth(self.handle, d_disp, count, fx, baseline, doffs, d_depth))

    def depth_from_both(self, d_disp_left: int, d_disp_right: int, count: int, fx_left: float, fx_right: float, baseline: float,
                        doffs: float, d_depth: int) -> bool:
        """sgm_depth_from_both: the left map's depth where finite, else the right map's at the same pixel (device pointers)."""
        return bool(self.lib.sgm_depth_from_both(self.handle, d_disp_left, d_disp_right, count, fx_left, fx_right, baseline, doffs,
                                                 d_depth))

    # ---- point clouds (include/sgm_mi355x.h, sgm_cloud_spec); device pointers as ints, None = NULL ----
    def cloud_organized(self, spec: SGMCloudSpec, d_disp, d_mask, d_conf, d_xyz: int) -> bool:
        """sgm_cloud_organized: float32 [frames][H][W][3], X Y Z of the kept pixels and NaN elsewhere.  d_disp None: the final map
        of the last match; d_mask (uint8) / d_conf (uint16) None: no such test.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_cloud_organized(self.handle, C.byref(spec), d_disp or None, d_mask or None, d_conf or None, d_xyz))

    def cloud_points(self, spec: SGMCloudSpec, d_disp, d_mask, d_conf, d_points: int, d_offsets: int) -> bool:
        """sgm_cloud_points: the kept pixels as 16-byte records in raster order (room for frames * H * W of them) and
        uint32 offsets [frames + 1].  Arguments as cloud_organized.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_cloud_points(self.handle, C.byref(spec), d_disp or None, d_mask or None, d_conf or None, d_points,
                                              d_offsets))

    def read_cloud(self, spec: SGMCloudSpec):
        """sgm_read_cloud: (points as POINT_DTYPE records, offsets uint32 [frames + 1]) of the last match's final map, no mask,
        no confidence; blocking.  None where the C call returns false."""
        return _read_cloud(lambda *a: self.lib.sgm_read_cloud(self.handle, *a), spec)

    # ---- depth registered to another camera (include/sgm_mi355x.h, sgm_register_spec); device pointers as ints, None = NULL ----
    def register_depth(self, src: SGMCloudSpec, dst: SGMRegisterSpec, d_disp, d_mask, d_conf, d_depth: int, d_source=None) -> bool:
        """sgm_register_depth: the kept pixels of the source map, z-buffered into the target camera: float32 depth
        [frames][dst.height][dst.width] (NaN where nothing landed) and, when asked, the uint32 source pixel (y << 16) | x of every
        winner (REGISTER_NONE elsewhere).  d_disp None: the final map of the last match.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_register_depth(self.handle, C.byref(src), C.byref(dst), d_disp or None, d_mask or None, d_conf or None,
                                                d_depth, d_source or None))

    def register_gather(self, src: SGMCloudSpec, dst: SGMRegisterSpec, d_source: int, d_map: int, d_out: int, dtype, fill=0) -> bool:
        """sgm_register_gather: a map of the source's shape (elements of dtype: 1, 2 or 4 bytes) carried into the target image through
        register_depth's source; `fill` where nothing landed.  Asynchronous on `stream`."""
        value = np.array([fill]).astype(np.dtype(dtype))
        return bool(self.lib.sgm_register_gather(self.handle, C.byref(src), C.byref(dst), d_source, value.itemsize, d_map,
                                                 value.ctypes.data, d_out))

    # ---- depth fused into a TSDF volume (include/sgm_mi355x.h, sgm_volume_spec); device pointers as ints, None = NULL ----
    def volume_integrate(self, spec: SGMVolumeSpec, src: SGMCloudSpec, poses, d_disp, d_mask, d_conf, d_voxels: int) -> bool:
        """sgm_volume_integrate: the kept pixels of src.frames maps fused into the volume at d_voxels (volume_bytes(spec) bytes, all
        zero when empty).  poses: [frames][12] (or [frames][3][4]) host floats, R row-major then t (world -> camera), read before the
        call returns.  d_disp None: the final map of the last match.  Asynchronous on `stream`."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if poses.size != 12 * src.frames:
            raise ValueError("volume_integrate: one pose of 12 floats (R row-major, then t) per frame")
        return bool(self.lib.sgm_volume_integrate(self.handle, C.byref(spec), C.byref(src), poses.ctypes.data, d_disp or None,
                                                  d_mask or None, d_conf or None, d_voxels))

    def volume_points(self, spec: SGMVolumeSpec, d_voxels: int, min_weight: int, d_points, capacity: int, d_count: int) -> bool:
        """sgm_volume_points: the zero crossings of the volume as SURFACE_DTYPE records sorted by id into d_points (16-byte aligned,
        room for `capacity` records; None with capacity 0) and their full number into d_count[0].  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_points(self.handle, C.byref(spec), d_voxels, int(min_weight), d_points or None, int(capacity),
                                               d_count))

    def volume_mesh(self, spec: SGMVolumeSpec, d_voxels: int, min_weight: int, d_vertices, vertex_capacity: int, d_triangles,
                    triangle_capacity: int, d_counts: int) -> bool:
        """sgm_volume_mesh: the volume as an indexed triangle mesh, marching tetrahedra: MESH_VERTEX_DTYPE records sorted by id into
        d_vertices and MESH_TRIANGLE_DTYPE records into d_triangles (both 16-byte aligned, may be None with capacity 0), the full
        numbers of vertices and triangles in d_counts[0], d_counts[1]; triangles only where the whole vertex list fitted"""
        return bool(self.lib.sgm_volume_mesh(self.handle, C.byref(spec), d_voxels, int(min_weight), d_vertices or None, int(vertex_capacity),
                                             d_triangles or None, int(triangle_capacity), d_counts))

    def volume_raycast(self, vol: SGMVolumeSpec, view: SGMRaycastSpec, poses, d_voxels: int, d_depth: int, d_normal=None) -> bool:
        """sgm_volume_raycast: the volume at d_voxels rendered into view.frames depth maps [frames][height][width] float32 at d_depth
        and, with d_normal, unit normals [frames][height][width][3] in camera coordinates; empty pixels hold the quiet NaN.  poses:
        [frames][12] host floats, R row-major then t (world -> camera), read before the call returns.  Asynchronous on `stream`."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if poses.size != 12 * view.frames:
            raise ValueError("volume_raycast: one pose of 12 floats (R row-major, then t) per frame")
        return bool(self.lib.sgm_volume_raycast(self.handle, C.byref(vol), C.byref(view), poses.ctypes.data, d_voxels, d_depth,
                                                d_normal or None))

    # ---- colour in the TSDF volume (include/sgm_mi355x.h, the colour section); device pointers as ints, None = NULL ----
    def volume_integrate_color(self, spec: SGMVolumeSpec, src: SGMCloudSpec, poses, d_disp, d_mask, d_conf, d_image: int, channels: int,
                               d_voxels: int, d_colors: int) -> bool:
        """sgm_volume_integrate_color: volume_integrate with the reference camera's image ([frames][height][width]: uint8 grey with
        channels 1, uint32 r | g << 8 | b << 16 with channels 4) fused into the colour words at d_colors (volume_bytes(spec) bytes,
        all zero when empty) by the same launch.  Asynchronous on `stream`."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if poses.size != 12 * src.frames:
            raise ValueError("volume_integrate_color: one pose of 12 floats (R row-major, then t) per frame")
        return bool(self.lib.sgm_volume_integrate_color(self.handle, C.byref(spec), C.byref(src), poses.ctypes.data, d_disp or None,
                                                        d_mask or None, d_conf or None, d_image or None, int(channels), d_voxels,
                                                        d_colors or None))

    def volume_raycast_color(self, vol: SGMVolumeSpec, view: SGMRaycastSpec, poses, d_voxels: int, d_colors: int, d_depth: int,
                             d_normal, d_rgba: int) -> bool:
        """sgm_volume_raycast_color: volume_raycast with the colour at every hit, 0xFF000000 | b << 16 | g << 8 | r, into d_rgba
        (uint32 [frames][height][width]; 0 for an empty pixel or a hit without colour).  Asynchronous on `stream`."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if poses.size != 12 * view.frames:
            raise ValueError("volume_raycast_color: one pose of 12 floats (R row-major, then t) per frame")
        return bool(self.lib.sgm_volume_raycast_color(self.handle, C.byref(vol), C.byref(view), poses.ctypes.data, d_voxels,
                                                      d_colors or None, d_depth, d_normal or None, d_rgba or None))

    def volume_colors(self, spec: SGMVolumeSpec, d_voxels: int, d_colors: int, d_records, capacity: int, d_count, id_kinds: int,
                      d_rgba) -> bool:
        """sgm_volume_colors: a colour (uint32 into d_rgba[r]) for each of the first `capacity` records at d_records -- the vertices
        of volume_mesh (id_kinds 8) or the points of volume_points (id_kinds 4) -- and, with d_count (a device uint32, e.g. the
        d_counts of volume_mesh), only for those below d_count[0].  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_colors(self.handle, C.byref(spec), d_voxels, d_colors or None, d_records or None, int(capacity),
                                               d_count or None, int(id_kinds), d_rgba or None))

    # ---- a window of the volume (include/sgm_mi355x.h, the window section); device pointers as ints, None = NULL ----
    def volume_window(self, src: SGMVolumeSpec, offset, dims, d_src_voxels: int, d_src_colors, d_dst_voxels: int, d_dst_colors=None):
        """sgm_volume_window: the `dims` voxels of `src` from `offset` on copied into the volume at d_dst_voxels (and the colour
        words into d_dst_colors where both colour arrays are given), 0 where the source has nothing.  Returns the window's spec,
        None where the call was refused.  Asynchronous on `stream`."""
        dst = SGMVolumeSpec()
        ok = self.lib.sgm_volume_window(self.handle, C.byref(src), _int3(offset, "volume_window"), _int3(dims, "volume_window"),
                                        d_src_voxels or None, d_src_colors or None, d_dst_voxels or None, d_dst_colors or None, C.byref(dst))
        return dst if ok else None

    # ---- the distance field of the volume (include/sgm_mi355x.h, the distance section); device pointers as ints, None = NULL ----
    def volume_distance(self, spec: SGMVolumeSpec, dist: SGMDistanceSpec, d_voxels: int, d_dist2: int) -> bool:
        """sgm_volume_distance: per voxel the squared distance, in voxels, to the nearest site of `dist` as uint16 into d_dist2
        (volume_distance_bytes(spec) bytes), DISTANCE_FAR beyond the radius.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_distance(self.handle, C.byref(spec), C.byref(dist), d_voxels or None, d_dist2 or None))

    def volume_distance_field(self, spec: SGMVolumeSpec, d_out2: int, d_in2, d_field: int) -> bool:
        """sgm_volume_distance_field: the metric field, float32 per voxel, from the side-0 words at d_out2 and, for the sign, the
        side-1 words at d_in2 (None: unsigned).  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_distance_field(self.handle, C.byref(spec), d_out2 or None, d_in2 or None, d_field or None))

    # ---- connected components of the volume (include/sgm_mi355x.h, the components section); device pointers as ints, None = NULL ----
    def volume_components(self, spec: SGMVolumeSpec, comp: SGMComponentSpec, d_voxels: int, d_labels: int, d_objects, capacity: int,
                          d_counts: int) -> bool:
        """sgm_volume_components: per voxel the label of its component (uint32 into d_labels, volume_components_bytes(spec) bytes:
        the smallest voxel index of the component plus 1, or 0), the first `capacity` surviving components as COMPONENT_DTYPE
        records into d_objects (None with capacity 0: labels and counts alone) and into d_counts the numbers of surviving and of all
        components.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_components(self.handle, C.byref(spec), C.byref(comp), d_voxels or None, d_labels or None,
                                                   d_objects or None, int(capacity), d_counts or None))

    def volume_component_of(self, spec: SGMVolumeSpec, d_labels: int, d_objects, capacity: int, d_counts: int, d_records, records_capacity: int,
                            d_records_count, id_kinds: int, d_index) -> bool:
        """sgm_volume_component_of: for each of the first `records_capacity` records at d_records (and d_records_count[0], where
        given) -- the vertices of volume_mesh with id_kinds 8, the points of volume_points with 4 -- 1 plus the position of its
        object in the list volume_components wrote, or 0, as uint32 into d_index.  Asynchronous on `stream`."""
        return bool(self.lib.sgm_volume_component_of(self.handle, C.byref(spec), d_labels or None, d_objects or None, int(capacity),
                                                     d_counts or None, d_records or None, int(records_capacity), d_records_count or None,
                                                     int(id_kinds), d_index or None))

    # ---- frame-to-model tracking (include/sgm_mi355x.h, sgm_track_spec); device pointers as ints, None = NULL ----
    def track_sums(self, src: SGMCloudSpec, model: SGMTrackSpec, poses, d_disp, d_mask, d_conf, d_model_depth: int, d_model_normal: int,
                   d_sums: int) -> bool:
        """sgm_track_sums: the 29 int64 sums of every frame into d_sums ([frames][29], 8-byte aligned) for the kept pixels of src
        moved by poses ([frames][12] host floats, source camera -> model camera, read before the call returns) against the model
        maps as volume_raycast writes them.  d_disp None: the final map of the last match.  Asynchronous on `stream`."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if poses.size != 12 * src.frames:
            raise ValueError("track_sums: one pose of 12 floats (R row-major, then t) per frame")
        return bool(self.lib.sgm_track_sums(self.handle, C.byref(src), C.byref(model), poses.ctypes.data, d_disp or None, d_mask or None,
                                            d_conf or None, d_model_depth, d_model_normal, d_sums))

    def track(self, src: SGMCloudSpec, model: SGMTrackSpec, poses, d_disp, d_mask, d_conf, d_model_depth: int, d_model_normal: int,
              trace: bool = False):
        """sgm_track (blocking): model.iterations rounds from the guess `poses` ([frames][12] doubles) -> (the estimate, float64
        [frames][12]; a list of dicts of pixels, rms and status per frame), with trace=True also the sums of every round (int64
        [iterations][frames][29]) and the poses before and after every round (float64 [iterations + 1][frames][12]).  None for a
        refused or failed call."""
        poses = np.array(poses, np.float64).reshape(-1)
        if poses.size != 12 * src.frames:
            raise ValueError("track: one pose of 12 doubles (R row-major, then t) per frame")
        stats = (SGMTrackStats * src.frames)()
        n = max(int(model.iterations), 0)
        t_sums = np.zeros((n, src.frames, 29), np.int64) if trace else None
        t_poses = np.zeros((n + 1, src.frames, 12), np.float64) if trace else None
        if not self.lib.sgm_track(self.handle, C.byref(src), C.byref(model), poses.ctypes.data, d_disp or None, d_mask or None,
                                  d_conf or None, d_model_depth, d_model_normal, C.addressof(stats),
                                  t_sums.ctypes.data if trace else None, t_poses.ctypes.data if trace else None):
            return None
        out = [dict(pixels=int(st.pixels), rms=float(st.rms), status=int(st.status)) for st in stats]
        return (poses.reshape(src.frames, 12), out, t_sums, t_poses) if trace else (poses.reshape(src.frames, 12), out)

    # ---- planes in a point list (include/sgm_mi355x.h, sgm_plane_spec); device pointers as ints, None = NULL ----
    def plane_votes(self, spec: SGMPlaneSpec, d_records: int, capacity: int, d_count, d_labels, d_planes: int) -> bool:
        """sgm_plane_votes: spec.hypotheses candidate planes from hashed triples of the 16-byte records at d_records (the first
        min(capacity, d_count[0]) of them; d_count None: capacity) and, for each, the exact number of its inliers, into d_planes
        (sgm_plane [hypotheses], 16-byte aligned).  d_labels (u8 per record, None: none) takes labelled records out.  Asynchronous
        on `stream`."""
        return bool(self.lib.sgm_plane_votes(self.handle, C.byref(spec), d_records or None, int(capacity), d_count or None, d_labels or None,
                                             d_planes or None))

    def plane_best(self, d_planes: int, k: int, d_best: int) -> bool:
        """sgm_plane_best: the candidate with the most votes (ties: the smallest index; all void: a void plane) into d_best."""
        return bool(self.lib.sgm_plane_best(self.handle, d_planes or None, int(k), d_best or None))

    def plane_sums(self, spec: SGMPlaneSpec, d_records: int, capacity: int, d_count, d_labels, d_plane: int, d_sums: int) -> bool:
        """sgm_plane_sums: the ten int64 moments of the inliers of the plane at d_plane into d_sums (8-byte aligned).  Asynchronous."""
        return bool(self.lib.sgm_plane_sums(self.handle, C.byref(spec), d_records or None, int(capacity), d_count or None, d_labels or None,
                                            d_plane or None, d_sums or None))

    def plane_label(self, spec: SGMPlaneSpec, d_records: int, capacity: int, d_count, d_plane: int, label: int, d_labels: int) -> bool:
        """sgm_plane_label: `label` (1..255) into d_labels[r] of every unlabelled inlier of the plane at d_plane.  Asynchronous."""
        return bool(self.lib.sgm_plane_label(self.handle, C.byref(spec), d_records or None, int(capacity), d_count or None, d_plane or None,
                                             int(label), d_labels or None))

    def plane_fit(self, spec: SGMPlaneSpec, d_records: int, capacity: int, d_count=None, d_labels=None, trace: bool = False):
        """sgm_plane_fit (blocking): vote, take the best candidate, refine it in spec.iterations rounds -> (the plane, a PLANE_DTYPE
        record; a dict of inliers, rms and status), with trace=True also the sums of every round (int64 [iterations][10]) and the
        planes before and after every round (PLANE_DTYPE [iterations + 1]).  None for a refused or failed call."""
        n = max(int(spec.iterations), 0)
        plane, st = SGMPlane(), SGMPlaneStats()
        t_sums = np.zeros((n, 10), np.int64) if trace else None
        t_planes = np.zeros(n + 1, PLANE_DTYPE) if trace else None
        if not self.lib.sgm_plane_fit(self.handle, C.byref(spec), d_records or None, int(capacity), d_count or None, d_labels or None,
                                      C.addressof(plane), C.addressof(st), t_sums.ctypes.data if trace else None,
                                      t_planes.ctypes.data if trace else None):
            return None
        out = _plane_record(plane), dict(inliers=int(st.inliers), rms=float(st.rms), status=int(st.status))
        return out + (t_sums, t_planes) if trace else out

    # ---- matching at 1/f scale (include/sgm_mi355x.h, sgm_scale_spec); device pointers as ints, None = NULL ----
    def downscale(self, spec: SGMScaleSpec, d_in: int, d_out: int) -> bool:
        """sgm_downscale: the f x f box mean of one image stack [frames][H][W] -> [frames][H / f][W / f].  Asynchronous on `stream`."""
        return bool(self.lib.sgm_downscale(self.handle, C.byref(spec), d_in, d_out))

    def upscale_disparity(self, spec: SGMScaleSpec, d_disp_small: int, d_guide_small: int, d_guide_full: int, d_census_ref,
                          d_census_oth, right_view: bool, d_disp_full: int) -> bool:
        """sgm_upscale_disparity: the guided selection and the re-search on the full-resolution census planes (None with a negative
        radius).  Asynchronous on `stream`."""
        return bool(self.lib.sgm_upscale_disparity(self.handle, C.byref(spec), d_disp_small, d_guide_small, d_guide_full,
                                                   d_census_ref or None, d_census_oth or None, 1 if right_view else 0, d_disp_full))

    def match_scaled(self, spec: SGMScaleSpec, left, right):
        """sgm_match_scaled: FULL-resolution images ([H][W], or [frames][H][W] with a batch) through an instance initialised at the
        low-resolution shape; the full-resolution float32 map, or None where the C call returns false."""
        left, right = self._img(left, spec.bits), self._img(right, spec.bits)
        want = (spec.height, spec.width) if spec.frames == 1 and left.ndim == 2 else (spec.frames, spec.height, spec.width)
        if tuple(left.shape) != want or tuple(right.shape) != want:
            raise ValueError(f"expected images of shape {want}, got {left.shape} and {right.shape}")
        out = np.empty(want, np.float32)
        ok = self.lib.sgm_match_scaled(self.handle, C.byref(spec), left.ctypes.data, right.ctypes.data, out.ctypes.data)
        return out if ok else None

    def match_scaled_device(self, spec: SGMScaleSpec, d_left: int, d_right: int, d_out: int) -> bool:
        """sgm_match_scaled_device: the same on device buffers, asynchronous on `stream`."""
        return bool(self.lib.sgm_match_scaled_device(self.handle, C.byref(spec), d_left, d_right, d_out))

    def compare_depth(self, d_ground_truth: int, d_test: int, count: int, abs_thresh: float = 10.0):
        """(rmse, bad_pixel_rate, n_valid) of two device depth images; None where the C call returns false."""
        rmse, bpr, n = C.c_double(), C.c_double(), C.c_uint64()
        ok = self.lib.sgm_compare_depth(self.handle, d_ground_truth, d_test, count, abs_thresh, C.byref(rmse), C.byref(bpr), C.byref(n))
        return (rmse.value, bpr.value, int(n.value)) if ok else None

    # ---- a test-platform frame end to end (include/sgm_mi355x.h) ----
    def gray_from_planes(self, d_bgr: int, count: int, d_gray: int, weight_r: int = 76) -> bool:
        """Device pointers: three `count`-byte planes B, G, R -> grey bytes; asynchronous on the instance stream."""
        return bool(self.lib.sgm_gray_from_planes(self.handle, d_bgr, count, weight_r, d_gray))

    def match_planes(self, planes, fx: float, baseline: float, doffs: float, depth, wait: bool = True) -> bool:
        """sgm_match_planes(_async): `planes` uint8 [batch *] 6 x H x W (left B, G, R, right B, G, R), `depth` float32 H x W per
        frame; with wait=False the arrays must stay alive and untouched until match_wait()."""
        for a in (planes, depth):
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError("match_planes needs C-contiguous arrays")
        if planes.dtype != np.uint8 or depth.dtype != np.float32:
            raise TypeError("match_planes: uint8 planes, float32 depth")
        if self.shape is None:
            return False
        h, w = self.shape[:2]
        if planes.size != self.batch * 6 * h * w or tuple(planes.shape[-2:]) != (h, w):
            raise ValueError(f"match_planes: planes of shape {tuple(planes.shape)}, expected [{self.batch} x] 6 x {h} x {w}")
        if depth.size != self.batch * h * w or tuple(depth.shape[-2:]) != (h, w):
            raise ValueError(f"match_planes: depth of shape {tuple(depth.shape)}, expected [{self.batch} x] {h} x {w}")
        fn = self.lib.sgm_match_planes if wait else self.lib.sgm_match_planes_async
        return bool(fn(self.handle, planes.ctypes.data, fx, baseline, doffs, depth.ctypes.data))

    @property
    def stream(self) -> int:
        return self.lib.sgm_stream(self.handle) or 0

    def _read(self, idx, out):
        return self.lib.sgm_read_stage(self.handle, idx, out.ctypes.data, out.nbytes)
