"""Depth from both views' maps (include/sgm_mi355x.h, sgm_depth_from_both): the host restatement
soc_project_stereo_matching_amd/platform.py against vectors the REFERENCE'S OWN FUNCTION produced -- depth_image.py:167-197,
depth_from_left_and_right_disp, compiled from the reference's text by tests/golden/make_golden_depth_both.py
(tests/golden/platform_depth_both.npz).  The device kernel is checked against the same vectors in test_gpu_match_both.py."""
import numpy as np

from conftest import load_npz
from soc_project_stereo_matching_amd.platform import depth_from_both, disparity_to_depth

PAIRS = ("cone", "random", "edge")


def fixture_cases():
    """(what, disp_left, disp_right, fx_left, fx_right, baseline, doffs, reference depth) for every stored pair, with the invalid
    pixels once as +INF (the library's marker, as stored) and once as NaN (the platform's, depth_image.py:130).  The library treats
    the two alike, so the expected image is in both cases what the reference's function returned for the NaN-masked maps."""
    z = load_npz("platform_depth_both.npz")
    for c in ("a", "b", "c"):
        fx_l, fx_r, baseline, doffs = (float(v) for v in z[f"calib_{c}"])
        for m in PAIRS:
            dl, dr = z[f"disp_left_{m}"], z[f"disp_right_{m}"]
            ref = z[f"depth_{c}_{m}_nan"]
            yield f"{c}/{m}/inf", dl, dr, fx_l, fx_r, baseline, doffs, ref
            yield (f"{c}/{m}/nan", np.where(np.isinf(dl), np.float32(np.nan), dl), np.where(np.isinf(dr), np.float32(np.nan), dr),
                   fx_l, fx_r, baseline, doffs, ref)


def check_against_reference(got, ref, what):
    """Exactly equal, bit for bit, wherever the reference's depth is finite; where it is not (no usable denominator in either map,
    or a quotient that overflows with nothing to fill it from) the library's is not finite either -- NaN here, NaN or +-inf there."""
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(got[fin].view(np.uint32), ref[fin].view(np.uint32)), what
    assert not np.isfinite(got[~fin]).any(), what


def test_host_restatement_equals_the_references_own_function():
    n = 0
    for what, dl, dr, fx_l, fx_r, baseline, doffs, ref in fixture_cases():
        check_against_reference(depth_from_both(dl, dr, fx_l, fx_r, baseline, doffs), ref, what)
        n += 1
    assert n == 18


def test_fixture_covers_the_fill_and_two_focal_lengths():
    z = load_npz("platform_depth_both.npz")
    assert z["calib_c"][0] != z["calib_c"][1] and z["calib_a"][0] == z["calib_a"][1]
    for m in PAIRS:
        dl, dr = z[f"disp_left_{m}"], z[f"disp_right_{m}"]
        filled = np.isinf(dl) & np.isfinite(dr)
        assert filled.any() and (np.isinf(dl) & np.isinf(dr)).any() and np.isfinite(dl).any(), m
        # the pixels taken from the right map carry the right camera's focal length
        fx_l, fx_r, baseline, doffs = (float(v) for v in z["calib_c"])
        ref = z[f"depth_c_{m}_nan"]
        right_only = disparity_to_depth(dr, fx_r, baseline, doffs)
        ok = filled & np.isfinite(ref)
        assert np.array_equal(ref[ok].view(np.uint32), right_only[ok].view(np.uint32)), m


def test_the_references_bare_formula_on_the_inf_marker():
    """What the reference's function returns for maps that carry this library's +INF marker unmasked: depth 0 at an invalid left
    pixel (finite, so never filled), and the NaN-masked result everywhere else.  The library does not follow it there: an invalid
    left pixel takes the right view's depth, as with the maps the platform feeds the function."""
    z = load_npz("platform_depth_both.npz")
    for c in ("a", "b", "c"):
        for m in PAIRS:
            dl = z[f"disp_left_{m}"]
            r_inf, r_nan = z[f"depth_{c}_{m}_inf"], z[f"depth_{c}_{m}_nan"]
            left_inf = np.isinf(dl)
            assert (r_inf[left_inf] == 0).all(), (c, m)
            both_fin = ~left_inf & np.isfinite(r_nan)
            assert np.array_equal(r_inf[both_fin].view(np.uint32), r_nan[both_fin].view(np.uint32)), (c, m)


def test_no_warping_between_the_views():
    """The fill is per pixel: the right map's value of the SAME pixel, whatever its disparity says about where it belongs."""
    dl = np.array([[np.inf, 10.0, np.inf, np.inf]], np.float32)
    dr = np.array([[20.0, 30.0, np.inf, 40.0]], np.float32)
    got = depth_from_both(dl, dr, 1000.0, 2000.0, 100.0, 0.0)
    assert got[0, 0] == np.float32(200000.0) / np.float32(20.0) and got[0, 1] == np.float32(100000.0) / np.float32(10.0)
    assert np.isnan(got[0, 2]) and got[0, 3] == np.float32(200000.0) / np.float32(40.0)


def test_the_two_restatements_of_the_depth_formula_agree():
    """The package's disparity_to_depth and the CPU checker's (oracle/platform_oracle.py) are the same arithmetic stated twice (the
    product does not import test infrastructure): bit-identical on every stored map and calibration."""
    from oracle.platform_oracle import disparity_to_depth as checker
    z = load_npz("platform_depth_both.npz")
    for c in ("a", "b", "c"):
        fx_l, fx_r, baseline, doffs = (float(v) for v in z[f"calib_{c}"])
        for m in PAIRS:
            for d in (z[f"disp_left_{m}"], z[f"disp_right_{m}"]):
                for fx in (fx_l, fx_r):
                    a, b = disparity_to_depth(d, fx, baseline, doffs), checker(d, fx, baseline, doffs)
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (c, m)
