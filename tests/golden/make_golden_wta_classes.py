#!/usr/bin/env python3
"""The planted winner-take-all inputs of tests/wta_classes.py: per-view class counts from the oracle's S, and every stage's
digest as the REFERENCE'S OWN C (oracle/_ref, guarded build) computes it beside the oracle's.  Run where the reference is present:

    make -C oracle ref && python tests/golden/make_golden_wta_classes.py      -> tests/golden/wta_classes.json

Inputs come from seeds (tests/wta_classes.py: INPUTS), so the file holds counts and digests only.  A combination the reference
cannot run without undefined behaviour (min_disparity > 0 with the LR check on and the uniqueness test off: it reads
cost_local[65535 - dmin], see _cases() in tests/test_oracle_vs_reference.py) is marked "oracle_only" and carries no reference
digests."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import wta_classes as WC  # noqa: E402
from oracle.pyoracle import STAGE_NAMES, Reference, sha  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wta_classes.json")


def reference_can_run(p):
    o = p.option
    return not (o.min_disparity > 0 and o.is_check_lr and not o.is_check_unique)


def q14_entry(name):
    """A sequence of matches without Reset (tests/q14_deep.py): counts from the oracle's S after the last match; the reference
    runs the same calls through its public entry points, which hand out the final map only."""
    p = WC.q14_planted(name)
    w, h, dmin, dmax = p.shape
    counts = p.counts()
    ref = Reference.for_shape(w, h, dmax - dmin)
    assert ref is not None
    for k, (l, r) in enumerate(p.frames):
        out = ref.api_match(l, r, p.option, reset=(k == 0))
        assert out is not None
    return {"matches": p.n, "shape": [w, h, dmin, dmax], "options": p.option_kw, "floor": WC.floor(w, h), "counts": counts,
            "planted": {v: [n for n in WC.CLASSES if counts[v][n] >= WC.floor(w, h)] for v in WC.VIEWS},
            "sha256_inputs": {"left": sha(p.frames[-1][0]), "right": sha(p.frames[-1][1])},
            "oracle_stages": {n: sha(p.stages[n]) for n in WC.Q14_STAGES + ("final",)},
            "oracle_only": False, "reference": os.path.basename(ref.path), "reference_stages": {"final": sha(out)}}


def main():
    doc = {"generator": "tests/golden/make_golden_wta_classes.py",
           "source": "class counts: tests/wta_classes.py on the oracle's S; reference_stages: oracle/_ref (reference C), ref_run_stages",
           "inputs": {}}
    for shape, variant, seed in WC.INPUTS:
        p = WC.planted(shape, variant, seed)
        w, h, dmin, dmax = p.shape
        counts = p.counts()
        e = {"seed": seed, "shape": [w, h, dmin, dmax], "options": p.option_kw, "bands": p.ks, "floor": WC.floor(w, h),
             "counts": counts,
             "planted": {v: [n for n in WC.CLASSES if counts[v][n] >= WC.floor(w, h)] for v in WC.VIEWS},
             "sha256_inputs": {"left": sha(p.left), "right": sha(p.right)},
             "oracle_stages": {n: sha(p.stages[n]) for n in STAGE_NAMES},
             "oracle_only": not reference_can_run(p), "reference": None, "reference_stages": None}
        if reference_can_run(p):
            ref = Reference.for_shape(w, h, dmax - dmin)
            assert ref is not None, f"no oracle/_ref build covers {w}x{h}x{dmax - dmin}: make -C oracle ref first"
            out = ref.run(p.left, p.right, p.option)
            e["reference"] = os.path.basename(ref.path)
            e["reference_stages"] = {n: sha(out[n]) for n in STAGE_NAMES}
        doc["inputs"][p.name] = e
    for name in WC.Q14_INPUTS:
        doc["inputs"][name] = q14_entry(name)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    n_ref = sum(1 for e in doc["inputs"].values() if not e["oracle_only"])
    print(f"wrote {OUT}: {len(doc['inputs'])} inputs, {n_ref} with reference digests")


if __name__ == "__main__":
    main()
