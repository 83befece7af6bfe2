#!/usr/bin/env python3
"""Digests of the cases of tests/limits.py -- the limits sgm_initialize admits -- produced by the REFERENCE ITSELF:

    python tests/golden/make_golden_limits.py          parts A, B and D (a minute)        -> tests/golden/limits.json "cases"
    python tests/golden/make_golden_limits.py --big    part C (2 to 3 minutes and up to 15 GB resident per case) -> ... "big"

The capacities these shapes need are built here with oracle/build_ref.sh where oracle/_ref/ does not hold them yet (they stay
out of the Makefile's REF_SHAPES: nothing but this generator needs them).  Expected values come from the reference's own
SemiGlobalMatching.c (guarded build); every case is also run through our restatement and the two are asserted equal on every
stage -- through `after_lr` only where a frame is wider or taller than 32768: the reference's RemoveSpeckles keeps neighbour
coordinates in int16_t (SemiGlobalMatching.c:618-620), so its `after_speckle` / `final` are stored beside
the oracle's there ("sha256" holds what the library has to give, "reference_sha256" the reference's two maps).
Cases the reference does not define are listed under "oracle_only" with the reason."""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import limits as LM  # noqa: E402
from make_golden import opt_dict  # noqa: E402
from oracle.pyoracle import STAGE_NAMES, Oracle, Reference, ref_path, sha  # noqa: E402

OUT = os.path.join(HERE, "limits.json")


def reference_for(w, h, d, cap):
    """A compiled reference that holds the shape: one of `make -C oracle ref` where that does, else capacity cap = (W, H, D), built on
    demand.  (Not the smallest cover of oracle/_ref/ blindly: RemoveSpeckles keeps 5 bytes per pixel of the CAPACITY on the stack,
    and a build made for part C does not fit the default stack limit.)"""
    path = ref_path(w, h, d)
    if path is not None and Reference(path).capacity[0] * Reference(path).capacity[1] * 5 < 4 << 20:
        return Reference(path)
    path = os.path.join(ROOT, "oracle", "_ref", "libsgm_ref_%dx%dx%d.so" % tuple(cap))
    if not os.path.exists(path):
        subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh")] + [str(v) for v in cap])
    return Reference(path)


def capacity(w, h, d):
    if max(w, h) > 1500:                                     # part B: one build for the wide frames, one for the tall ones
        return (65535, 12, 128) if w > h else (12, 65535, 64)
    return (1400, 24, 512)                                   # part A: what `make -C oracle ref` does not cover


def compare(ref_st, orc_st, cut):
    """The stages on which the reference and the oracle have to agree: all, or through after_lr where the int16 cut applies."""
    for n in STAGE_NAMES:
        if cut and n in ("after_speckle", "final"):
            continue
        assert ref_st[n].dtype == orc_st[n].dtype and np.array_equal(ref_st[n].view(np.uint8), orc_st[n].view(np.uint8)), n


def one_frame(orc, left, right, opt, honor=False):
    h, w = left.shape
    d = opt.max_disparity - opt.min_disparity
    ref = reference_for(w, h, d, capacity(w, h, d))
    ref_st = ref.run(left, right, opt)
    orc.set_honor_num_paths(honor)
    orc_st = orc.run(left, right, opt)
    orc.set_honor_num_paths(False)
    cut = LM.beyond_int16(w, h)
    compare(ref_st, orc_st, cut)
    entry = {"sha256_inputs": {"left": sha(left), "right": sha(right)},
             "sha256": {n: sha(orc_st[n] if cut and n in ("after_speckle", "final") else ref_st[n]) for n in STAGE_NAMES},
             "finite_final": int(np.isfinite(orc_st["final"]).sum()), "finite_disp_r": int(np.isfinite(orc_st["disp_r"]).sum()),
             "oob_dropped": ref.oob_count()}
    if cut:
        entry["reference_sha256"] = {n: sha(ref_st[n]) for n in ("after_speckle", "final")}
        entry["differ_from_reference"] = {n: int((ref_st[n].view(np.uint32) != orc_st[n].view(np.uint32)).sum())
                                          for n in ("after_speckle", "final")}
    return entry


def small():
    orc = Oracle()
    cases = {}
    for c in LM.DMIN_CASES:
        opt = LM.dmin_option(c)
        frames = [one_frame(orc, *LM.dmin_pair(orc.synth_pair, c, f), opt) for f in range(3)]       # the GPU test's batch of 3
        cases[LM.dmin_name(c)] = {"part": "A", "shape": list(c), "option": opt_dict(opt), "frames": frames}
        if c in LM.DMIN_IN_RANGE:
            assert min(f["finite_final"] for f in frames) >= LM.DMIN_QUOTA, (c, frames[0]["finite_final"])
            assert min(f["finite_disp_r"] for f in frames) >= LM.DMIN_QUOTA, (c, frames[0]["finite_disp_r"])
        print(LM.dmin_name(c), [(f["finite_final"], f["finite_disp_r"]) for f in frames], flush=True)
    for c in LM.WIDE_CASES:
        opt = LM.wide_option(c)
        frames = [one_frame(orc, *LM.wide_pair(orc.synth_pair, c, f), opt) for f in range(c[4])]
        cases[LM.wide_name(c)] = {"part": "B", "shape": list(c), "option": opt_dict(opt), "frames": frames,
                                  "equal_to_reference_through": "after_lr" if LM.beyond_int16(c[0], c[1]) else "final"}
        print(LM.wide_name(c), [(f["finite_final"], f.get("differ_from_reference")) for f in frames], flush=True)
    left, right = LM.option_pair(orc.synth_pair)
    for name, (kw, honor, by_reference) in LM.OPTION_ENDS.items():
        opt = LM.option_of(name)
        if by_reference:
            frame = one_frame(orc, left, right, opt, honor)
        else:                                                # the oracle's digests, labelled: see "oracle_only"
            orc.set_honor_num_paths(honor)
            st = orc.run(left, right, opt)
            orc.set_honor_num_paths(False)
            frame = {"sha256_inputs": {"left": sha(left), "right": sha(right)}, "sha256": {n: sha(st[n]) for n in STAGE_NAMES},
                     "finite_final": int(np.isfinite(st["final"]).sum()), "finite_disp_r": int(np.isfinite(st["disp_r"]).sum())}
        cases["option_" + name] = {"part": "D", "shape": list(LM.OPTION_SHAPE), "option": opt_dict(opt), "honor_num_paths": honor,
                                   "by": "reference" if by_reference else "oracle", "note": LM.OPTION_NOTES.get(name, ""),
                                   "frames": [frame]}
        print("option_" + name, frame["finite_final"], flush=True)
    return cases


def big_case(name):
    """One case of part C in a process of its own (the reference's static buffers stay resident once touched)."""
    import resource
    # the reference's RemoveSpeckles keeps uint8 + uint32 [MAX_IMG_SIZE] on the stack (SemiGlobalMatching.c:588-589)
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    from oracle.pyoracle import default_option
    w, h, d, seed = LM.BIG_CASES[name]
    assert w * h * d < 2 ** 31 <= w * h * LM.padded_stride(d) < 2 ** 32
    orc = Oracle()
    left, right = orc.synth_pair(w, h, d, seed)
    opt = default_option(d)
    ref = reference_for(w, h, d, (w, h, d))
    t0 = time.time()
    st = ref.run(left, right, opt)
    t_ref = time.time() - t0
    entry = {"name": name, "w": w, "h": h, "d": d, "seed": seed, "option": opt_dict(opt), "padded_cells": w * h * LM.padded_stride(d),
             "real_cells": w * h * d, "oob_dropped": ref.oob_count(), "reference_seconds": round(t_ref, 1),
             "sha256": {n: sha(st[n]) for n in STAGE_NAMES}, "sha256_inputs": {"left": sha(left), "right": sha(right)},
             "invalid_final": int(np.isinf(st["final"]).sum()), "finite_disp_r": int(np.isfinite(st["disp_r"]).sum()),
             "aggr_sum": int(st["aggr"].sum(dtype=np.uint64)), "aggr_max": int(st["aggr"].max())}
    del st, ref
    t0 = time.time()
    orc.clear_census()
    assert orc.reset(w, h, opt) and orc.match(left, right) is not None
    entry["oracle_seconds"] = round(time.time() - t0, 1)
    for n in STAGE_NAMES:                                    # one stage at a time: `aggr` alone is 4 GB
        assert sha(orc.stage(n)) == entry["sha256"][n], f"{name}: the oracle's {n} differs from the reference's"
    entry["peak_rss_gb"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 1)
    print(json.dumps(entry), flush=True)


def load():
    if os.path.exists(OUT):
        with open(OUT) as f:
            return json.load(f)
    return {"generator": "tests/golden/make_golden_limits.py", "source": "oracle/_ref (reference C, guarded build)"}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--big-case":
        return big_case(sys.argv[2])
    if len(sys.argv) > 1 and sys.argv[1] == "--big":
        for name in (sys.argv[2:] or list(LM.BIG_CASES)):
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--big-case", name], text=True)
            doc = load()                                     # parts A, B and D may have been written meanwhile
            big = doc.setdefault("big", {})
            big[name] = json.loads(out.strip().splitlines()[-1])
            print(name, big[name]["reference_seconds"], "s reference,", big[name]["oracle_seconds"], "s oracle,",
                  big[name]["peak_rss_gb"], "GB", flush=True)
            with open(OUT, "w") as f:
                json.dump(doc, f, indent=1)
        return
    cases = small()
    doc = load()
    doc["cases"] = cases
    doc["oracle_only"] = LM.ORACLE_ONLY
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
