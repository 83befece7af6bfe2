"""What the temporal filter costs and what it buys (NOTES.md section 27) -- needs an MI355X.

    python tools/temporal_bench.py [--rounds 5] [--calls 40] [--warmup 5] [--parent-library PATH] [--out profiles/temporal_bench.txt]

KITTI 1242x375, D = 128, batch 8, device-resident.  One JSON line per case, also written to --out.

1. The filter alone (sgm_temporal_filter on the maps of a real match, by turns with the project's yardsticks for streaming kernels on
   the same maps, sgm_cloud_organized and sgm_disparity_to_depth): sequence = 0 (8 streams of one step) and sequence = 1 (one stream
   of 8 steps), with and without statistics.  Per round and case: `warmup` calls, then `calls` calls queued back to back between two
   HIP events on the instance's stream; time per call = elapsed / calls; median, minimum, maximum over the rounds.  Bytes a call
   must move: the maps read and written (8 B per pixel and step) and the history read and written once (10 B per pixel and stream).
2. The cost through the match: sgm_reset + sgm_match_device per batch, wall clock over `calls` queued calls, with the filter off, on
   and on with statistics, in alternating rounds.  Each leg is a process of its own (one library per process); with --parent-library
   (a build of the parent commit, e.g. tools/build_variant.sh from a checkout of it) the filter-off leg also runs on that build,
   alternating with this one.
3. Off must cost nothing: this build's filter-off median must lie inside the spread of the parent's own rounds, widened by 1 %
   for clock drift between alternating runs.  Printed as "off_inside_parent_spread".
4. Accuracy through the library on six frames (seeded +-3 grey levels of noise) of the cone pair and of the Middlebury scene Wood2
   against their ground truth (tests/golden/gt_disparity.npz), alpha 0.4, delta 1.0, for hold off and hold 2-of-3: on the pixels
   valid in the raw and the filtered map, the mean frame-to-frame change and the share of pixels off by more than 0.5 / 1 px, raw
   and filtered; and the held pixels' own count and error rate in the last frame."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--parent-library", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.txt"))
ap.add_argument("--leg", default=None, help="internal: off | on | stats -- one round of the match leg, prints ms per batch")
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
N = W * H * B

import numpy as np, torch
import soc_project_stereo_matching_amd as S


def kitti_batch():
    pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
    return torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(), torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()


def match_leg(leg):
    """ms per batch of sgm_reset + sgm_match_device, `rounds` rounds in this process"""
    l, r = kitti_batch()
    disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    opt = S.default_option(D)
    inst = S.SGMInstance(0, batch=B)
    if leg != "off":
        assert inst.set_temporal(S.temporal_spec(0.4, 1.0, 3, 2, stats=leg == "stats"))
    torch.cuda.synchronize()
    for _ in range(10):
        assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr())
    assert inst.synchronize()
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr())
        assert inst.synchronize()
        ms.append((time.perf_counter() - t0) / args.calls * 1e3)
    inst.close()
    return ms


if args.leg:
    print(json.dumps(match_leg(args.leg)))
    sys.exit(0)

lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


# ---- 1. the filter alone ---------------------------------------------------------------------------------------------------------
l, r = kitti_batch()
disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
inst = S.SGMInstance(0, batch=B)
assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()) and inst.synchronize()
raw = disp.clone()
hv = torch.empty(N, dtype=torch.float32, device="cuda")
hb = torch.empty(N, dtype=torch.uint8, device="cuda")
stats = torch.zeros(B * 5, dtype=torch.int32, device="cuda")
depth = torch.empty(N, dtype=torch.float32, device="cuda")
xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")
cspec = S.cloud_spec(W, H, 721.5377, 721.5377, 609.5593, 172.854, 0.54, 0.0, frames=B)
tspec = S.temporal_spec(0.4, 1.0, 3, 2)
px = W * H
filt = lambda streams, steps, st: inst.temporal_filter(tspec, streams, steps, px, disp.data_ptr(), None, hv.data_ptr(), hb.data_ptr(), st)
calls = {
    "sgm_disparity_to_depth": (lambda: inst.disparity_to_depth(raw.data_ptr(), N, cspec.fx, cspec.baseline, cspec.doffs, depth.data_ptr()), 8 * N),
    "sgm_cloud_organized": (lambda: inst.cloud_organized(cspec, raw.data_ptr(), None, None, xyz.data_ptr()), 16 * N),
    "temporal sequence=0": (lambda: filt(B, 1, None), 8 * N + 10 * N),
    "temporal sequence=0 stats": (lambda: filt(B, 1, stats.data_ptr()), 8 * N + 10 * N),
    "temporal sequence=1": (lambda: filt(1, B, None), 8 * N + 10 * px),
    "temporal sequence=1 stats": (lambda: filt(1, B, stats.data_ptr()), 8 * N + 10 * px),
}
stream = torch.cuda.ExternalStream(inst.stream)
us = {name: [] for name in calls}
assert inst.temporal_clear(B, px, hv.data_ptr(), hb.data_ptr())
for _ in range(args.rounds):
    for name, (call, _) in calls.items():
        for _ in range(args.warmup):
            assert call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            assert call()
        b.record(stream)
        b.synchronize()
        us[name].append(a.elapsed_time(b) / args.calls * 1e3)
assert inst.synchronize()
inst.close()
rate = {}
for name, (_, moved) in calls.items():
    med = statistics.median(us[name])
    rate[name] = moved / (med * 1e-6) / 1e9
    emit({"case": name, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
          "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls, "bytes_moved": moved, "GB_per_s": round(rate[name], 1)})
emit({"case": "byte rate against sgm_cloud_organized",
      **{name: round(rate[name] / rate["sgm_cloud_organized"], 3) for name in calls if name.startswith("temporal")}})
del l, r, disp, raw, hv, hb, depth, xyz
torch.cuda.empty_cache()

# ---- 2. / 3. the cost through the match, each leg a process of its own ----------------------------------------------------------------
legs = [("off", None), ("on", None), ("stats", None)] + ([("off", args.parent_library)] if args.parent_library else [])
ms = {leg: [] for leg in legs}
for turn in range(3):
    for leg in legs:
        env = dict(os.environ)
        if leg[1]:
            env["SGM_LIBRARY_PATH"] = os.path.abspath(leg[1])
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg[0], "--rounds", str(args.rounds), "--calls", str(args.calls)],
                             capture_output=True, text=True, env=env, timeout=600)
        if out.returncode != 0:
            raise SystemExit(f"leg {leg} failed: {out.stderr[-2000:]}")
        ms[leg] += json.loads(out.stdout.strip().splitlines()[-1])
for leg in legs:
    emit({"case": "match, filter " + leg[0] + (" (parent build)" if leg[1] else ""), "ms_per_batch_median": round(statistics.median(ms[leg]), 4),
          "min": round(min(ms[leg]), 4), "max": round(max(ms[leg]), 4), "rounds": [round(x, 4) for x in ms[leg]], "calls_per_round": args.calls})
off = statistics.median(ms[("off", None)])
emit({"case": "filter on against off", "on": round(statistics.median(ms[("on", None)]) / off, 4),
      "on_with_stats": round(statistics.median(ms[("stats", None)]) / off, 4)})
if args.parent_library:
    p = ms[("off", args.parent_library)]
    lo, hi = min(p) * 0.99, max(p) * 1.01
    emit({"case": "off must cost nothing", "off_median_ms": round(off, 4), "parent_spread_ms_widened_1_percent": [round(lo, 4), round(hi, 4)],
          "parent_median_ms": round(statistics.median(p), 4), "off_inside_parent_spread": bool(lo <= off <= hi)})

# ---- 4. accuracy through the library -------------------------------------------------------------------------------------------------
from conftest import case_inputs, load_npz, option_from_dict
from oracle.pyoracle import Oracle
import temporal_cases as TC

gt = load_npz("gt_disparity.npz")
orc = Oracle()
cases = {}
for name in ("cases.json", "cases_scenes.json"):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        cases.update({c["name"]: c for c in json.load(f)["cases"]})
for scene, case in (("cone", "cone"), ("wood2", "scene_wood2")):
    left, right = case_inputs(cases[case], orc)
    copt = option_from_dict(cases[case]["option"])
    truth, known = gt[scene].astype(np.float32) / gt[scene + "_scale"], gt[scene] > 0
    h, w = left.shape
    frames = TC.frames_of(left, right, blank=-1)
    plain = S.SGMInstance(0)
    raws = []
    for fl, fr in frames:
        assert plain.reset(w, h, copt)
        raws.append(plain.match(fl, fr))
    plain.close()
    for hold in ((0, 1), (3, 2)):
        inst = S.SGMInstance(0)
        assert inst.set_temporal(S.temporal_spec(0.4, 1.0, hold[0], hold[1]))
        outs = []
        for fl, fr in frames:
            assert inst.reset(w, h, copt)
            outs.append(inst.match(fl, fr))
        inst.close()
        both = [np.isfinite(a) & np.isfinite(b) for a, b in zip(raws, outs)]
        change = lambda maps: float(np.mean([np.abs(maps[k][m] - maps[k - 1][m]).mean() for k in range(1, len(maps))
                                             for m in [both[k] & both[k - 1]]]))
        last = both[-1] & known
        err = lambda m, t: round(100 * float((np.abs(m[last] - truth[last]) > t).mean()), 2)
        held = np.isfinite(outs[-1]) & ~np.isfinite(raws[-1]) & known
        emit({"case": f"accuracy {scene}, hold {hold[1]}-of-{hold[0]}" if hold[0] else f"accuracy {scene}, hold off",
              "mean_frame_to_frame_change_px": {"raw": round(change(raws), 4), "filtered": round(change(outs), 4)},
              "error_gt_0.5px_percent": {"raw": err(raws[-1], 0.5), "filtered": err(outs[-1], 0.5)},
              "error_gt_1px_percent": {"raw": err(raws[-1], 1.0), "filtered": err(outs[-1], 1.0)},
              "common_pixels_last_frame": int(last.sum()), "held_pixels_last_frame": int(held.sum()),
              "held_error_gt_1px_percent": round(100 * float((np.abs(outs[-1][held] - truth[held]) > 1).mean()), 2) if held.any() else None})
with open(args.out, "w") as f:
    f.write("python tools/temporal_bench.py --rounds %d --calls %d%s\n" % (args.rounds, args.calls, " --parent-library <a build of the parent commit>" if args.parent_library else ""))
    f.write("\n".join(lines) + "\n")
