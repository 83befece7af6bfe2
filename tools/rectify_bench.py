"""What rectification costs a call (NOTES.md section 19) -- needs an MI355X.

    python tools/rectify_bench.py [--rounds 7] [--calls 40] [--off-only]

KITTI 1242x375, D = 128, 8 paths, batch 8, device-resident frames.  One call = sgm_reset + sgm_match_device.  Three instances in
one process, visited by turns:
    off1, off2  rectification never set, twice: what separates them is the noise floor of the method
    on          the radial + rotation maps of tests/rectify_ref.py (SMALL), the two cameras rolled against each other
20 warm-up calls each, then `rounds` rounds of `calls` calls queued back to back and one synchronize, wall clock / calls.  Then,
in passes of their own: the mean device time of "census" over 20 calls per case with sgm_enable_timing (the remap counts toward
it), and the remap alone -- sgm_rectify queued 200 times back to back, wall clock / calls -- with the bytes it moves: each map entry
once per batch (2 views x 8 B x W x H), each image read and written once (2 views x B x 2 B x W x H).
--off-only: the off cases alone, for a build without the feature (SGM_LIBRARY_PATH names the library): the parent's number in
the same session.  Prints one JSON line per case and a last one with the differences."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--off-only", action="store_true")
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
names = ["off1", "off2"] if args.off_only else ["off1", "on", "off2"]
inst = {name: S.SGMInstance(0, batch=B) for name in names}
if not args.off_only:
    import rectify_ref as RR
    assert inst["on"].set_rectify(*RR.model_maps(RR.SMALL, W, H), *RR.model_maps(RR.SMALL, W, H, sign=-1.0))


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
census = {}
for name, i in inst.items():
    i.enable_timing(True)
    for _ in range(20):
        step(i)
    assert i.synchronize()
    mean, _, n = i.mean_timing()
    assert n == 20
    census[name] = round(mean["census"], 4)
    i.enable_timing(False)
med = {name: statistics.median(v) for name, v in rounds.items()}
for name in names:
    print(json.dumps({"case": name, "library": S.library_path(), "ms_per_batch_median": round(med[name], 4), "min": round(min(rounds[name]), 4),
                      "max": round(max(rounds[name]), 4), "rounds": [round(x, 4) for x in rounds[name]], "calls_per_round": args.calls,
                      "census_mean_ms": census[name], "valid_pixels": valid[name]}))
summary = {"noise_floor_ms": round(abs(med["off1"] - med["off2"]), 4), "off_ms": round((med["off1"] + med["off2"]) / 2, 4)}
if not args.off_only:
    i = inst["on"]
    rl, rr = torch.empty_like(l), torch.empty_like(r)
    torch.cuda.synchronize()
    alone = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(200):
            assert i.rectify(l.data_ptr(), r.data_ptr(), rl.data_ptr(), rr.data_ptr())
        assert i.synchronize()
        alone.append((time.perf_counter() - t0) / 200 * 1e3)
    moved = 2 * 8 * W * H + 2 * B * 2 * W * H
    k_ms = statistics.median(alone)
    summary.update({"on_ms": round(med["on"], 4), "on_minus_off_ms": round(med["on"] - summary["off_ms"], 4),
                    "on_over_off": round(med["on"] / summary["off_ms"], 4),
                    "census_on_minus_off_ms": round(census["on"] - (census["off1"] + census["off2"]) / 2, 4),
                    "remap_alone_ms": round(k_ms, 4), "remap_alone_min_ms": round(min(alone), 4), "remap_bytes": moved,
                    "remap_GB_per_s": round(moved / (k_ms * 1e-3) / 1e9, 1)})
print(json.dumps(summary))
for i in inst.values():
    i.close()
