"""soc_project_stereo_matching_amd -- MI355X-native Semi-Global Matching behind the reference's C boundary.

The product is ``libsgm_mi355x.so`` (C host + hand-written gfx950 HIP kernels, see ``csrc/``) whose
entry points are the reference's ``SGM_Initialize / SGM_Reset / SGM_Match``
(reference: SemiGlobalMatching/SemiGlobalMatching/SemiGlobalMatching.h:78-80).  This Python package
is only a ctypes mirror of that C interface for tests and benchmarks; it contains no compute and
has no CPU fallback -- importing works anywhere, calling into the library needs a gfx950 GPU.
"""
from .sgm import (SGM, SGMInstance, SGMOption, default_option, library_path, load_library,  # noqa: F401
                  STAGE_NAMES, synth_pair, set_refine, refine_table, REFINE_LAMBDA, REFINE_SIGMA, REFINE_ITERS,
                  rectify_maps, STAGE_RECT_LEFT, STAGE_RECT_RIGHT, SGMCloudSpec, POINT_DTYPE, cloud_spec, SGMRegisterSpec, REGISTER_NONE,
                  register_spec, register_spec_raw,
                  SGMVolumeSpec, SURFACE_DTYPE, MESH_VERTEX_DTYPE, MESH_TRIANGLE_DTYPE, SGMMeshVertex, SGMMeshTriangle, volume_spec, volume_bytes, SGMRaycastSpec, raycast_spec,
                  SGMVolumeBox, volume_window_spec, volume_follow, volume_leaving,
                  SGMDistanceSpec, DISTANCE_FAR, distance_spec, volume_distance_bytes,
                  SGMTrackSpec, SGMTrackStats, track_spec, track_solve, track_world_pose,
                  SGMPlane, SGMPlaneSpec, SGMPlaneStats, PLANE_DTYPE, plane_spec, plane_solve,
                  SGMComponentSpec, SGMComponent, COMPONENT_DTYPE, component_spec, volume_components_bytes, component_metric,
                  rectify_valid_mask, STAGE_NARROW_LEFT, STAGE_NARROW_RIGHT, SGMScaleSpec, scale_spec, scaled_shape,
                  SGMTemporalSpec, temporal_spec, TEMPORAL_CLASSES, STAGE_TEMPORAL_IN, STAGE_TEMPORAL_VALUE, STAGE_TEMPORAL_BITS,
                  debug_guard_check)
from .sharding import SGMStream, frames_of_rank, match_sharded  # noqa: F401

__all__ = ["SGM", "SGMInstance", "SGMOption", "default_option", "library_path", "load_library", "STAGE_NAMES",
           "synth_pair", "set_refine", "refine_table", "REFINE_LAMBDA", "REFINE_SIGMA", "REFINE_ITERS", "rectify_maps",
           "STAGE_RECT_LEFT", "STAGE_RECT_RIGHT", "SGMCloudSpec", "POINT_DTYPE", "cloud_spec", "SGMRegisterSpec", "REGISTER_NONE",
           "register_spec", "register_spec_raw", "SGMVolumeSpec", "SURFACE_DTYPE", "MESH_VERTEX_DTYPE", "MESH_TRIANGLE_DTYPE", "SGMMeshVertex", "SGMMeshTriangle", "volume_spec", "volume_bytes", "SGMRaycastSpec", "raycast_spec",
           "SGMVolumeBox", "volume_window_spec", "volume_follow", "volume_leaving",
           "SGMDistanceSpec", "DISTANCE_FAR", "distance_spec", "volume_distance_bytes",
           "SGMTrackSpec", "SGMTrackStats", "track_spec", "track_solve", "track_world_pose",
           "SGMPlane", "SGMPlaneSpec", "SGMPlaneStats", "PLANE_DTYPE", "plane_spec", "plane_solve",
           "SGMComponentSpec", "SGMComponent", "COMPONENT_DTYPE", "component_spec", "volume_components_bytes", "component_metric",
           "rectify_valid_mask",
           "STAGE_NARROW_LEFT", "STAGE_NARROW_RIGHT", "SGMScaleSpec", "scale_spec", "scaled_shape", "SGMTemporalSpec", "temporal_spec",
           "TEMPORAL_CLASSES", "STAGE_TEMPORAL_IN", "STAGE_TEMPORAL_VALUE", "STAGE_TEMPORAL_BITS", "debug_guard_check", "SGMStream", "frames_of_rank", "match_sharded"]
