#!/usr/bin/env python3
"""Golden vectors for the depth image the test platform builds from a left AND a right disparity map, produced by the REFERENCE'S
OWN FUNCTION: HostScript_Server/depth_image.py:167-197, depth_from_left_and_right_disp (which calls disparity_to_depth, :138-165).

The method is make_golden_depth.py's: depth_image.py cannot be imported (its first lines import cv2, not installed here, and no
stand-in is made), but the two functions are plain numpy.  This script (build container only) parses the file with `ast`, compiles
exactly those two FunctionDef nodes from the reference's text where it lies, and runs them on the reference's own
stereo_calibration.StereoCalib.  Nothing of the reference is copied: the repo gets arrays (tests/golden/platform_depth_both.npz).

Invalid pixels of the stored inputs carry +INF, the library's marker, as in make_golden_depth.py.  The reference's function is run
on every pair twice: on the maps as stored ("inf": its bare formula turns a +INF disparity into depth 0, which it counts as finite
and never fills) and with +INF replaced by NaN ("nan": how the platform itself masks invalid pixels before calling it,
depth_image.py:130 -- there an invalid left pixel is filled from the right map).  Both results are stored.

    python tests/golden/make_golden_depth_both.py
"""
import ast
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.environ.get("SGM_REFERENCE_DIR", "/root/reference"), "HostScript_Server")
sys.path.insert(0, ROOT)


def reference_functions():
    sys.path.insert(0, REF)
    import stereo_calibration                                   # noqa: E402  reference module (numpy only), never shipped
    with open(os.path.join(REF, "depth_image.py")) as f:
        tree = ast.parse(f.read())
    ns = {"np": np, "StereoCalib": stereo_calibration.StereoCalib}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("disparity_to_depth", "depth_from_left_and_right_disp"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), "depth_image.py", "exec"), ns)
    return stereo_calibration.StereoCalib, ns["depth_from_left_and_right_disp"]


def both_views(left, right, dmax):
    """the two finished maps of a pair by the repo's CPU oracle (left view, right view)"""
    from oracle.pyoracle import Oracle, default_option
    orc = Oracle()
    out = []
    for view in (False, True):
        orc.set_reference_view(view)
        out.append(orc.run(left, right, default_option(dmax))["final"])
    return out


def main():
    StereoCalib, ref_both = reference_functions()
    out = {"numpy_version": np.frombuffer(np.__version__.encode(), np.uint8)}
    calibs = {
        # make_golden_depth.py's two blocks (equal focal lengths) and one whose cameras differ in fx
        "a": "cam0=[1733.74 0 792.27; 0 1733.74 541.89; 0 0 1]\ncam1=[1733.74 0 792.27; 0 1733.74 541.89; 0 0 1]\ndoffs=0\nbaseline=536.62\nwidth=1920\nheight=1080\nndisp=170\n",
        "b": "cam0=[3979.911 0 1244.772; 0 3979.911 1019.507; 0 0 1]\ncam1=[3979.911 0 1369.115; 0 3979.911 1019.507; 0 0 1]\ndoffs=124.343\nbaseline=193.001\nwidth=2964\nheight=1988\nndisp=280\n",
        "c": "cam0=[1733.74 0 792.27; 0 1733.74 541.89; 0 0 1]\ncam1=[1741.13 0 801.5; 0 1741.13 541.89; 0 0 1]\ndoffs=31.5\nbaseline=536.62\nwidth=1920\nheight=1080\nndisp=170\n",
    }
    rng = np.random.default_rng(20261016)
    with np.load(os.path.join(OUT, "cone_inputs.npz")) as z:
        cone_l, cone_r = both_views(z["left"], z["right"], 64)
    rand_l = (rng.random((48, 97), dtype=np.float32) * 200).astype(np.float32)
    rand_r = (rng.random((48, 97), dtype=np.float32) * 200).astype(np.float32)
    rand_l[rng.random(rand_l.shape) < 0.3] = np.inf
    rand_r[rng.random(rand_r.shape) < 0.3] = np.inf
    edge = [0.0, -0.0, 1.0, 0.5, 127.75, 3.4028235e38, 1e-30, -5.0, np.inf, -124.343, -31.5, 63.99999]
    pairs = {
        "cone": (cone_l[120:280, 100:340].copy(), cone_r[120:280, 100:340].copy()),     # real maps of both views incl. +INF
        "random": (rand_l, rand_r),
        # every edge value on the left against every edge value on the right
        "edge": (np.repeat(np.array(edge, np.float32), len(edge))[None, :].copy(), np.tile(np.array(edge, np.float32), len(edge))[None, :].copy()),
    }
    n = 0
    for cname, txt in calibs.items():
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as tf:
            tf.write(txt)
        cal = StereoCalib(tf.name)
        cal.scale_calib(1280, 720)
        os.unlink(tf.name)
        assert isinstance(cal.cam0[0, 0], np.float32) and isinstance(cal.cam1[0, 0], np.float32)
        out[f"calib_{cname}"] = np.array([cal.cam0[0, 0], cal.cam1[0, 0], cal.baseline, cal.doffs], np.float64)
        for mname, (dl, dr) in pairs.items():
            out[f"disp_left_{mname}"], out[f"disp_right_{mname}"] = dl, dr
            for marker in ("inf", "nan"):
                a, b = dl.copy(), dr.copy()
                if marker == "nan":
                    a[np.isinf(a)] = np.nan
                    b[np.isinf(b)] = np.nan
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    d = ref_both(a, b, cal)
                assert d.dtype == np.float32, d.dtype
                out[f"depth_{cname}_{mname}_{marker}"] = d
            n += 1
    out["cases"] = np.array([n])
    np.savez_compressed(os.path.join(OUT, "platform_depth_both.npz"), **out)
    print("wrote platform_depth_both.npz:", n, "pairs x 2 markers; numpy", np.__version__)


if __name__ == "__main__":
    main()
