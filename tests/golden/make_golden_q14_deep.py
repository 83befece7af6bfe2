#!/usr/bin/env python3
"""A hundred SGM_Match calls after ONE SGM_Reset, through the reference's own entry points -- produced by the REFERENCE ITSELF.

SGM_Match adds every frame's path costs onto the uint16 volume that only SGM_Initialize / SGM_Reset clear: after
some 25 matches cells pass 32768, where the reference's (int16) casts in the sub-pixel step start to matter, after some 50 the
sums wrap.  This script runs the sequences of tests/q14_deep.py (frames, shapes, checkpoints: defined there) through
SGM_Reset once and SGM_Match N times and records what came out:

    make -C oracle ref && python tests/golden/make_golden_q14_deep.py
        -> tests/golden/q14_deep.json           per shape and match: sha256 of the final map, number of invalid pixels
        -> tests/golden/q14_deep_<shape>.npz    the full final maps at the checkpoints (final_<match>)

Expected values come from oracle/_ref/libsgm_ref_*.so (the reference's SemiGlobalMatching.c, guarded build); our CPU restatement
supplies the seeded input generator only.  The .npz members are stored uncompressed with a fixed timestamp, so the files come out
byte for byte the same on every run."""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0))
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    import q14_deep as Q
    from oracle.pyoracle import Oracle, Reference, default_option, sha
    gen = Oracle()                                                # input generator only
    shapes = {}
    for name, (w, h, dmin, dmax) in Q.FIXTURE_SHAPES.items():
        ref = Reference.for_shape(w, h, dmax - dmin)
        assert ref is not None, f"no reference build covers {w}x{h}x{dmax - dmin}; run `make -C oracle ref`"
        opt = default_option(dmax, dmin, min_speckle_area=Q.FIXTURE_SPECKLE_AREA)
        matches, maps = [], {}
        for k in range(Q.N):
            l, r = Q.frame(gen.synth_pair, w, h, dmin, dmax, Q.BASE, k)
            out = ref.api_match(l, r, opt, reset=(k == 0))       # S keeps every earlier frame's sums
            assert out is not None
            matches.append({"sha256": sha(out), "invalid": int(np.isinf(out).sum())})
            if k in Q.FIXTURE_CHECKPOINTS[name]:
                maps[f"final_{k}"] = out
        write_npz(os.path.join(OUT, f"q14_deep_{name}.npz"), maps)
        shapes[name] = {"w": w, "h": h, "dmin": dmin, "dmax": dmax, "base": Q.BASE, "n": Q.N,
                        "min_speckle_area": Q.FIXTURE_SPECKLE_AREA, "checkpoints": list(Q.FIXTURE_CHECKPOINTS[name]),
                        "reference": os.path.basename(ref.path), "matches": matches}
    with open(os.path.join(OUT, "q14_deep.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_q14_deep.py",
                   "sequence": "tests/q14_deep.py: SGM_Reset once, then SGM_Match n times", "shapes": shapes}, f, indent=1)
        f.write("\n")
    print("wrote q14_deep.json and", ", ".join(f"q14_deep_{n}.npz" for n in shapes))


if __name__ == "__main__":
    main()
