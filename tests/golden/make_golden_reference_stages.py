#!/usr/bin/env python3
"""Golden digests for tests/test_oracle_vs_reference.py, made by the REFERENCE'S OWN C (oracle/_ref, guarded build).

For every case of that test: the sha256, shape and dtype of each of the nine stages the reference computes (ref_run_stages), and for
its per-direction cases the cost volume and each direction's aggregation (ref_aggregate_dir).  Run where the reference is present:

    make -C oracle ref && python tests/golden/make_golden_reference_stages.py      -> tests/golden/reference_stages.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle.pyoracle import DIRECTIONS, STAGE_NAMES, Oracle, Reference, default_option, sha  # noqa: E402
from test_oracle_vs_reference import AGG_CASES, _cases, agg_id, case_id  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_stages.json")


def entry(a):
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": sha(a)}


def main():
    gen = Oracle()                                 # the seeded input generator (the same LCG as the reference's harness)
    doc = {"generator": "tests/golden/make_golden_reference_stages.py",
           "source": "oracle/_ref (reference C, guarded build): ref_run_stages, ref_aggregate_dir", "cases": {}, "aggregate_dir": {}}
    for case in _cases():
        w, h, dmin, dmax, seed, kw = case
        ref = Reference.for_shape(w, h, dmax - dmin)
        assert ref is not None, f"no oracle/_ref build covers {w}x{h}x{dmax - dmin}: make -C oracle ref first"
        left, right = gen.synth_pair(w, h, dmax - dmin, seed)
        out = ref.run(left, right, default_option(dmax, dmin, **kw))
        doc["cases"][case_id(case)] = {"options": kw, "sha256_inputs": {"left": sha(left), "right": sha(right)},
                                       "reference": os.path.basename(ref.path), "stages": {n: entry(out[n]) for n in STAGE_NAMES}}
    for (w, h, d, seed) in AGG_CASES:
        ref = Reference.for_shape(w, h, d)
        left, right = gen.synth_pair(w, h, d, seed)
        opt = default_option(d)
        cost = ref.run(left, right, opt)["cost"]
        doc["aggregate_dir"][agg_id((w, h, d, seed))] = {
            "sha256_inputs": {"left": sha(left), "right": sha(right)}, "reference": os.path.basename(ref.path), "cost": entry(cost),
            "directions": {f"{dx},{dy}": entry(ref.aggregate_dir(left, cost, opt, dx, dy)) for dx, dy in DIRECTIONS}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['cases'])} cases, {len(doc['aggregate_dir'])} per-direction cases")


if __name__ == "__main__":
    main()
