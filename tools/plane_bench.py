"""What finding a plane in a point list costs a call (NOTES.md section 42) -- needs an MI355X.

    python tools/plane_bench.py [--rounds 7] [--calls 20] [--warmup 3] [--label lane-counters]

The set-up of tools/track_bench.py: KITTI 1242x375, D = 128, batch 8, device-resident, the disparity maps of a real match of
SGM_SynthPair frames, and their cloud list (sgm_cloud_points: all eight frames, one list with its count word).  By turns:
sgm_plane_votes with 64, 256 and 1024 candidates (half-thickness 0.1 m), sgm_plane_best of 1024, sgm_plane_sums and sgm_plane_label
at the best plane, and as yardsticks in the same run sgm_cloud_points, sgm_track_sums of the eight frames (against the frames' own
depth with a constant normal: every kept pixel is associated) and the match itself.  The method of measuring-on-mi355x as section
29 applies it: per round and call `warmup` calls, then `calls` calls queued back to back between two HIP events on the instance's
stream; time per call = elapsed / calls.  sgm_plane_fit blocks (a vote, the best plane, a copy of 32 bytes, then per round a launch,
a copy of 80 bytes, a wait and the solve), so it is timed with the host's clock.  Median, minimum and maximum over the rounds.
Prints one JSON line per call; the vote's rows carry its rate in point-plane tests per second.  --label names the build in the
output (SGM_LIBRARY_PATH may point at the library of another build)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="lane-counters")
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
N = W * H * B
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
inst = S.SGMInstance(0, batch=B)
assert inst.reset(W, H, S.default_option(D)) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()) and inst.synchronize()

FX, FY, CX, CY, BASELINE = 721.5377, 721.5377, 609.5593, 172.854, 0.54
src = S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B, z_max=80.0)
points = torch.zeros(4 * N, dtype=torch.float32, device="cuda")
offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
labels = torch.zeros(N, dtype=torch.uint8, device="cuda")
planes = torch.zeros(8 * 1024, dtype=torch.float32, device="cuda")
best = torch.zeros(8, dtype=torch.float32, device="cuda")
sums = torch.zeros(10, dtype=torch.int64, device="cuda")
assert inst.cloud_points(src, disp.data_ptr(), None, None, points.data_ptr(), offsets.data_ptr()) and inst.synchronize()
count = offsets.data_ptr() + 4 * B
n = int(offsets.cpu().numpy()[B])
spec = {k: S.plane_spec(k, 0.1, 20.0, seed=1, iterations=4, min_inliers=100, min_pivot=1e-9) for k in (64, 256, 1024)}

# the yardstick of tracking: the frames against their own depth, normals facing the camera
xyz = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
assert inst.cloud_organized(src, disp.data_ptr(), None, None, xyz.data_ptr()) and inst.synchronize()
depth = xyz[..., 2].contiguous()
normal = torch.zeros((B, H, W, 3), dtype=torch.float32, device="cuda")
normal[..., 2] = -1.0
model = S.track_spec(W, H, FX, FY, CX, CY, 0.5, 20.0, iterations=1, min_pixels=1000, min_pivot=1e-9)
identity = np.zeros((B, 12), np.float32)
identity[:, [0, 4, 8]] = 1.0
track_sums = torch.zeros(B * 29, dtype=torch.int64, device="cuda")


def votes(k):
    return inst.plane_votes(spec[k], points.data_ptr(), N, count, None, planes.data_ptr())


assert votes(1024) and inst.plane_best(planes.data_ptr(), 1024, best.data_ptr()) and inst.synchronize()
found = np.frombuffer(best.cpu().numpy().tobytes(), S.PLANE_DTYPE)[0]
fitted = inst.plane_fit(spec[1024], points.data_ptr(), N, count, None)
assert fitted is not None
shape = {"records": n, "capacity": N, "best_of_1024": {"votes": int(found["votes"]), "normal": [round(float(v), 4) for v in found["normal"]]},
         "fit_4_rounds": dict(fitted[1], normal=[round(float(v), 4) for v in fitted[0]["normal"]], offset=round(float(fitted[0]["offset"]), 4))}

queued = {
    "sgm_plane_votes K = 64": lambda: votes(64),
    "sgm_plane_votes K = 256": lambda: votes(256),
    "sgm_plane_votes K = 1024": lambda: votes(1024),
    "sgm_plane_best K = 1024": lambda: inst.plane_best(planes.data_ptr(), 1024, best.data_ptr()),
    "sgm_plane_sums": lambda: inst.plane_sums(spec[64], points.data_ptr(), N, count, None, best.data_ptr(), sums.data_ptr()),
    "sgm_plane_label": lambda: inst.plane_label(spec[64], points.data_ptr(), N, count, best.data_ptr(), 1, labels.data_ptr()),
    "sgm_cloud_points": lambda: inst.cloud_points(src, disp.data_ptr(), None, None, points.data_ptr(), offsets.data_ptr()),
    "sgm_track_sums 8 frames": lambda: inst.track_sums(src, model, identity, disp.data_ptr(), None, None, depth.data_ptr(), normal.data_ptr(),
                                                       track_sums.data_ptr()),
    "match (batch of 8, device pointers)": lambda: inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()),
}
blocking = {
    "sgm_plane_fit K = 64, 4 rounds": lambda: inst.plane_fit(spec[64], points.data_ptr(), N, count, None),
    "sgm_plane_fit K = 1024, 4 rounds": lambda: inst.plane_fit(spec[1024], points.data_ptr(), N, count, None),
}

stream = torch.cuda.ExternalStream(inst.stream)
us = {name: [] for name in list(queued) + list(blocking)}
for _ in range(args.rounds):
    for name, call in queued.items():
        if name == "sgm_plane_label":
            labels.zero_()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            assert call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            assert call()
        b.record(stream)
        b.synchronize()
        us[name].append(a.elapsed_time(b) / args.calls * 1e3)
    for name, call in blocking.items():
        for _ in range(args.warmup):
            assert call() is not None
        t0 = time.perf_counter()
        for _ in range(args.calls):
            assert call() is not None
        us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
assert inst.synchronize()
for name in us:
    med = statistics.median(us[name])
    row = {"case": name, "label": args.label, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
           "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls, "clock": "host" if name in blocking else "HIP events"}
    if name.startswith("sgm_plane_votes"):
        k = int(name.split("=")[1])
        row["point_plane_tests"] = n * k
        row["tests_per_second"] = round(n * k / (med * 1e-6), 0)
    print(json.dumps(row))
print(json.dumps({"case": "the list and its plane", "label": args.label, **shape}))
inst.close()
