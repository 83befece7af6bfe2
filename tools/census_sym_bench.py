"""What a wide census window costs on the two routes to it (NOTES.md section 18) -- needs an MI355X.

    python tools/census_sym_bench.py [--rounds 7] [--calls 40]

KITTI 1242x375, D = 128, 8 paths, batch 8, device-resident frames.  One call = sgm_reset + sgm_match_device.  Five instances in
one process, one per case:
    a1, a2  centre 5x5 (the reference's census) twice: what separates them is the noise floor of the method
    b       centre 9x7: u64 words, a materialised cost volume, the volume-fed aggregation
    c       symmetric 9x7 (SGM_SetCensusKind): u32 words on the fast path
    d       symmetric 7x7, the drivers' default window for that kind
20 warm-up calls each, then `rounds` rounds that visit the cases by turns: `calls` calls queued back to back and one synchronize,
wall clock / calls.  Then, in a pass of its own with sgm_enable_timing, the mean device time of "census", "cost" and "aggregate"
over 20 calls per case.  Prints one JSON line per case and a last one with the differences the design predicts."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import soc_project_stereo_matching_amd as S
from soc_project_stereo_matching_amd import sgm

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=40)
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
CASES = [("a1", sgm.CENSUS_CENTRE, (5, 5)), ("b", sgm.CENSUS_CENTRE, (9, 7)), ("c", sgm.CENSUS_SYMMETRIC, (9, 7)),
         ("d", sgm.CENSUS_SYMMETRIC, sgm.CENSUS_SYMMETRIC_WINDOW), ("a2", sgm.CENSUS_CENTRE, (5, 5))]
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
inst = {}
for name, kind, (cw, ch) in CASES:
    inst[name] = i = S.SGMInstance(0, batch=B)
    assert i.set_census_kind(kind) and i.set_census_window(cw, ch)


def step(i):
    assert i.reset(W, H, opt) and i.match_device(l.data_ptr(), r.data_ptr(), out.data_ptr())


valid = {}
for name, i in inst.items():
    for _ in range(20):
        step(i)
    assert i.synchronize()
    valid[name] = int(torch.isfinite(out).sum())
rounds = {name: [] for name in inst}
for _ in range(args.rounds):
    for name, i in inst.items():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            step(i)
        assert i.synchronize()
        rounds[name].append((time.perf_counter() - t0) / args.calls * 1e3)
stages = {}
for name, i in inst.items():
    i.enable_timing(True)
    for _ in range(20):
        step(i)
    assert i.synchronize()
    mean, _, n = i.mean_timing()
    assert n == 20
    stages[name] = {k: round(mean[k], 4) for k in ("census", "cost", "aggregate", "sum")}
    i.enable_timing(False)
med = {name: statistics.median(v) for name, v in rounds.items()}
for name, kind, (cw, ch) in CASES:
    print(json.dumps({"case": name, "census": ("symmetric" if kind else "centre") + f" {cw}x{ch}",
                      "ms_per_batch_median": round(med[name], 4), "min": round(min(rounds[name]), 4), "max": round(max(rounds[name]), 4),
                      "rounds": [round(x, 4) for x in rounds[name]], "calls_per_round": args.calls, "stage_mean_ms": stages[name],
                      "valid_pixels": valid[name]}))
floor = abs(med["a1"] - med["a2"])
base = (med["a1"] + med["a2"]) / 2
print(json.dumps({"noise_floor_ms": round(floor, 4), "centre_5x5_ms": round(base, 4),
                  "c_minus_a_ms": round(med["c"] - base, 4), "c_census_minus_a_census_ms": round(stages["c"]["census"] - stages["a1"]["census"], 4),
                  "d_minus_a_ms": round(med["d"] - base, 4), "d_census_minus_a_census_ms": round(stages["d"]["census"] - stages["a1"]["census"], 4),
                  "b_minus_a_ms": round(med["b"] - base, 4), "c_over_a": round(med["c"] / base, 4), "d_over_a": round(med["d"] / base, 4),
                  "b_over_a": round(med["b"] / base, 4)}))
for i in inst.values():
    i.close()
