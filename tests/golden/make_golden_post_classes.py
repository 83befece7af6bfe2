#!/usr/bin/env python3
"""The planted inputs of tests/post_classes.py for the LR checks, the classification and the fill passes: digests of the inputs
and of every expected output, and the census counts.  Made from the restatements alone -- the oracle's two LR checks and
tests/fill_holes_ref.py -- without the library:

    python tests/golden/make_golden_post_classes.py      -> tests/golden/post_classes.json

Inputs come from seeds (tests/post_classes.py: LR_INPUTS, FILL_INPUTS), so the file holds digests and counts only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fill_holes_ref as F  # noqa: E402
import post_classes as PC  # noqa: E402
from oracle.pyoracle import Oracle, sha  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "post_classes.json")


def lr_entry(oracle, name):
    p = PC.lr_input(name)
    both = PC.lr_both(oracle, p.dl, p.dr, p.thres)
    return {"seed": p.seed, "shape": [p.W, p.H, PC.B], "options": {"lrcheck_thres": p.thres, "kind": p.kind},
            "sha256_inputs": {"disp_l": sha(p.dl), "disp_r": sha(p.dr)},
            "sha256_outputs": {"lr_left": sha(PC.lr_left(oracle, p.dl, p.dr, p.thres)), "lr_right": sha(PC.lr_right(oracle, p.dr, p.dl, p.thres)),
                               "lr_both_left": sha(both[0]), "lr_both_right": sha(both[1]),
                               "classes_left": sha(PC.classes(p.dl, p.dr, p.thres, False)),
                               "classes_right": sha(PC.classes(p.dr, p.dl, p.thres, True))},
            "counts": p.counts()}


def fill_entry(shape, variant):
    p = PC.fill_input(shape, variant)
    e = {"seed": p.seed, "shape": [p.W, p.H, PC.B], "options": {"variant": variant, "R": list(PC.FILL_RS)},
         "sha256_inputs": {"disp": sha(p.disp), "classes": sha(p.cls)}, "sha256_outputs": {}, "counts": {}}
    for R in PC.FILL_RS:
        p1, p2, p3 = PC.fill_passes(p.disp, p.cls, R)
        e["sha256_outputs"][str(R)] = {"pass1": sha(p1), "pass2": sha(p2), "pass3": sha(p3), "fill": sha(F.fill(p.disp, p.cls, R)),
                                       "fill_without_classes": sha(F.fill(p.disp, None, R))}
        e["counts"][str(R)] = p.counts(R)
    return e


def document():
    oracle = Oracle()
    return {"generator": "tests/golden/make_golden_post_classes.py",
            "source": "oracle sgmo_lrcheck / sgmo_lrcheck_right, tests/fill_holes_ref.py; counts: tests/post_classes.py census / fill_census",
            "floor": PC.FLOOR,
            "lr": {name: lr_entry(oracle, name) for name in PC.LR_INPUTS},
            "fill": {f"{s}-{v}": fill_entry(s, v) for s, v in PC.FILL_INPUTS}}


def main():
    with open(OUT, "w") as f:
        json.dump(document(), f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
