#!/usr/bin/env python3
"""Ground truth of the reference's four image pairs (tests/test_refine_cpu.py scores maps against it):
Data/cone/disp2.png (the left view im2 of Middlebury 2003 `cones`, quarter size) and Data/{Cloth3,Reindeer,Wood2}/disp1.png (the
left view view1 of Middlebury 2006, as the reference ships them).  Committed as one npz, gt_disparity.npz: per scene the u8 map as
stored (<scene>) and its scale (<scene>_scale, f32): disparity = value / scale, value 0 = unknown.

cone: the Middlebury 2003 quarter-size convention, disparity = value / 4.  The other three: the scale is established from the data,
not assumed -- the median of value / disparity over the pixels where the oracle's final map (the reference's options, the committed
grey inputs of make_golden_scenes.py) is finite and the ground truth known, rounded to the nearest integer; the raw median is kept
as <scene>_scale_measured.

Run in the build container (needs /root/reference):

    python tests/golden/make_golden_gt.py

Images are data files of the reference, stored as arrays -- no source text.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.pyoracle import Oracle  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
DATA = "/root/reference/SemiGlobalMatching/Data/"
SCENES = {"cone": "cone/disp2.png", "cloth3": "Cloth3/disp1.png", "reindeer": "Reindeer/disp1.png", "wood2": "Wood2/disp1.png"}


def main():
    from PIL import Image
    from conftest import option_from_dict
    with open(os.path.join(OUT, "cases_scenes.json")) as f:
        cases = {c["name"]: c for c in json.load(f)["cases"]}
    orc = Oracle()
    out = {}
    for name, path in SCENES.items():
        gt = np.asarray(Image.open(DATA + path), np.uint8)
        assert gt.ndim == 2, (path, gt.shape)
        out[name] = gt
        if name == "cone":
            out[name + "_scale"] = np.float32(4.0)
            continue
        case = cases["scene_" + name]
        with np.load(os.path.join(OUT, case["inputs_file"])) as z:
            left, right = z["left"], z["right"]
        final = orc.run(left, right, option_from_dict(case["option"]))["final"]
        ok = np.isfinite(final) & (gt > 0) & (final > 1)
        measured = float(np.median(gt[ok].astype(np.float64) / final[ok]))
        out[name + "_scale"] = np.float32(round(measured))
        out[name + "_scale_measured"] = np.float32(measured)
        print(f"{name}: scale measured {measured:.4f} over {int(ok.sum())} pixels -> {round(measured)}")
    np.savez_compressed(os.path.join(OUT, "gt_disparity.npz"), **out)
    print("wrote", os.path.join(OUT, "gt_disparity.npz"), os.path.getsize(os.path.join(OUT, "gt_disparity.npz")), "bytes")


if __name__ == "__main__":
    main()
