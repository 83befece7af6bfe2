"""What a point cloud costs a call (NOTES.md section 21) -- needs an MI355X.

    python tools/cloud_bench.py [--rounds 9] [--calls 40] [--warmup 5]

KITTI 1242x375, D = 128, batch 8, device-resident: the disparity maps of a real match of SGM_SynthPair frames.  Three calls on that
map, by turns: sgm_disparity_to_depth (the yardstick: the element-wise kernel over the same pixels), sgm_cloud_organized and
sgm_cloud_points.  Per round and call: `warmup` calls, then `calls` calls queued back to back between two HIP events on the
instance's stream; time per call = elapsed / calls.  Median, minimum and maximum over the rounds.  Bytes a call must move: depth
4 + 4 B/px; organised 4 + 12 B/px; list 2 x 4 B/px read + 16 B per kept point.  Prints one JSON line per call and the match's own
time per batch (sgm_reset + sgm_match_device, wall clock over `calls` queued calls) beside them."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
N = W * H * B
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
inst = S.SGMInstance(0, batch=B)


def match():
    assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr())


for _ in range(10):
    match()
assert inst.synchronize()
match_ms = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    for _ in range(args.calls):
        match()
    assert inst.synchronize()
    match_ms.append((time.perf_counter() - t0) / args.calls * 1e3)

spec = S.cloud_spec(W, H, 721.5377, 721.5377, 609.5593, 172.854, 0.54, 0.0, frames=B)
depth = torch.empty(N, dtype=torch.float32, device="cuda")
xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")
points = torch.empty(4 * N, dtype=torch.float32, device="cuda")
offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
calls = {
    "sgm_disparity_to_depth": lambda: inst.disparity_to_depth(disp.data_ptr(), N, spec.fx, spec.baseline, spec.doffs, depth.data_ptr()),
    "sgm_cloud_organized": lambda: inst.cloud_organized(spec, disp.data_ptr(), None, None, xyz.data_ptr()),
    "sgm_cloud_points": lambda: inst.cloud_points(spec, disp.data_ptr(), None, None, points.data_ptr(), offsets.data_ptr()),
}
stream = torch.cuda.ExternalStream(inst.stream)
us = {name: [] for name in calls}
for _ in range(args.rounds):
    for name, call in calls.items():
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
kept = int(offsets.cpu().numpy().view(np.uint32)[-1])
finite = int(torch.isfinite(disp).sum())
moved = {"sgm_disparity_to_depth": 8 * N, "sgm_cloud_organized": 16 * N, "sgm_cloud_points": 8 * N + 16 * kept}
print(json.dumps({"case": "match", "ms_per_batch_median": round(statistics.median(match_ms), 4), "min": round(min(match_ms), 4),
                  "max": round(max(match_ms), 4), "pixels": N, "finite_disparities": finite, "kept_points": kept,
                  "kept_share": round(kept / N, 4)}))
for name in calls:
    med = statistics.median(us[name])
    print(json.dumps({"case": name, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
                      "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls, "bytes_moved": moved[name],
                      "GB_per_s": round(moved[name] / (med * 1e-6) / 1e9, 1),
                      "share_of_match": round(med * 1e-3 / statistics.median(match_ms), 4)}))
inst.close()
