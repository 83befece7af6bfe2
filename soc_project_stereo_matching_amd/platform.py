"""Host restatement of the test-platform arithmetic the library runs on device buffers (include/sgm_mi355x.h, "test-platform
arithmetic"): what sgm_disparity_to_depth and sgm_depth_from_both compute, in numpy, for callers whose maps are on the host and for
the tests that pin the device kernels.

Arithmetic (float32 throughout, as on the device): the product fx * baseline is formed once and rounded to float32; depth is one
correctly rounded float32 divide by the float32 sum disparity + doffs; a non-finite or zero denominator gives NaN (the invalid
marker of a disparity map is +INF).
`disparity_to_depth` states the same arithmetic as the tests' CPU checker oracle/platform_oracle.py (test infrastructure the product
may not import); tests/test_depth_both_cpu.py holds the two to each other bit for bit, so they cannot drift apart unnoticed.

The module shares its name with the standard library's `platform`; it is only ever imported through the package
(`soc_project_stereo_matching_amd.platform`), never with the package directory on sys.path.
"""
from __future__ import annotations

import numpy as np


def disparity_to_depth(disp, fx, baseline, doffs):
    """Depth in millimetres of a float32 disparity map (sgm_disparity_to_depth)."""
    d = np.asarray(disp, dtype=np.float32)
    scale = np.float32(float(np.float32(fx)) * float(np.float32(baseline)))       # one rounding of the product
    denom = d + np.float32(doffs)
    usable = np.isfinite(denom) & (denom != 0)
    out = np.full(d.shape, np.nan, dtype=np.float32)
    np.divide(scale, denom, out=out, where=usable)
    return out


def depth_from_both(disp_left, disp_right, fx_left, fx_right, baseline, doffs):
    """sgm_depth_from_both: the test platform's depth image from a left and a right map (HostScript_Server/depth_image.py:167-197,
    depth_from_left_and_right_disp): the left map's depth with fx_left (cam0[0,0]) where that is finite, else the right map's depth
    with fx_right (cam1[0,0]) of the SAME pixel.  No warping between the views: the reference's behaviour, kept."""
    depth_l = disparity_to_depth(disp_left, fx_left, baseline, doffs)
    depth_r = disparity_to_depth(disp_right, fx_right, baseline, doffs)
    return np.where(np.isfinite(depth_l), depth_l, depth_r)
