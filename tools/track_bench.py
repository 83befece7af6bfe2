"""What frame-to-model tracking costs a call (NOTES.md section 35) -- needs an MI355X.

    python tools/track_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label atomics]

The set-up of tools/raycast_bench.py: KITTI 1242x375, D = 128, batch 8, device-resident, the disparity maps of a real match of
SGM_SynthPair frames fused (sgm_volume_integrate, B = 8) into 512 x 128 x 512 voxels of 0.1 m (134 MB) in front of the rig, eight
poses advancing 0.5 m along Z, and the volume ray-cast with normals into the 1242x375 view of every pose.  By turns: sgm_track_sums
of frame 0 and of all eight frames against those renders, from a pose 5 cm off the identity (gate 0.5 m, span 20 m), and as
yardsticks sgm_volume_raycast of one view with normals and sgm_cloud_organized.  The method of section 29: per round and call
`warmup` calls, then `calls` calls queued back to back between two HIP events on the instance's stream; time per call = elapsed /
calls.  sgm_track blocks (per round: a launch, a copy of 232 bytes per frame, a wait, the solve), so it is timed with the host's
clock over `calls` calls of 1 and of 4 rounds.  Median, minimum and maximum over the rounds.  Prints one JSON line per call.
--label names the build in the output (SGM_LIBRARY_PATH may point at the library of another commit)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="atomics")
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
NX, NY, NZ, VOXEL, TRUNC = 512, 128, 512, 0.1, 0.4
Z_MIN, Z_MAX, STEP = 0.5, 55.0, 0.2
vol = S.volume_spec(NX, NY, NZ, VOXEL, (-0.5 * NX * VOXEL, -0.5 * NY * VOXEL, 2.0), TRUNC, max_weight=64)
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src = {f: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=f) for f in (1, B)}
view = {f: S.raycast_spec(W, H, FX, FY, CX, CY, Z_MIN, Z_MAX, STEP, 1, frames=f) for f in (1, B)}
model = {it: S.track_spec(W, H, FX, FY, CX, CY, 0.5, 20.0, iterations=it, min_pixels=1000, min_pivot=1e-9) for it in (1, 4)}
guess = np.zeros((B, 12), np.float64)
guess[:, [0, 4, 8]] = 1.0
guess[:, 9] = 0.05                                                # the source camera 5 cm beside the model camera

voxels = torch.zeros(NX * NY * NZ, dtype=torch.int32, device="cuda")
depth = torch.empty(N, dtype=torch.float32, device="cuda")
normal = torch.empty(3 * N, dtype=torch.float32, device="cuda")
scratch_depth = torch.empty(W * H, dtype=torch.float32, device="cuda")      # what the ray-cast yardstick writes
scratch_normal = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")
sums = torch.zeros(B * 29, dtype=torch.int64, device="cuda")
assert inst.volume_integrate(vol, src[B], poses, disp.data_ptr(), None, None, voxels.data_ptr())
assert inst.volume_raycast(vol, view[B], poses, voxels.data_ptr(), depth.data_ptr(), normal.data_ptr()) and inst.synchronize()


def track_sums(frames):
    return inst.track_sums(src[frames], model[1], guess[:frames].astype(np.float32), disp.data_ptr(), None, None, depth.data_ptr(),
                           normal.data_ptr(), sums.data_ptr())


def track(frames, rounds):
    return inst.track(src[frames], model[rounds], guess[:frames], disp.data_ptr(), None, None, depth.data_ptr(), normal.data_ptr())


assert track_sums(B) and inst.synchronize()
associated = sums.cpu().numpy().reshape(B, 29)[:, 28].tolist()
tracked = track(B, 4)
assert tracked is not None
shape = {"associated_pixels": associated, "pixels_per_frame": W * H,
         "after_4_rounds": [dict(st, tx=round(float(p[9]), 5)) for p, st in zip(tracked[0], tracked[1])]}

queued = {
    "sgm_track_sums 1 frame": lambda: track_sums(1),
    "sgm_track_sums 8 frames": lambda: track_sums(B),
    "sgm_volume_raycast 1 view, depth + normals": lambda: inst.volume_raycast(vol, view[1], poses[:1], voxels.data_ptr(), scratch_depth.data_ptr(),
                                                                              scratch_normal.data_ptr()),
    "sgm_cloud_organized": lambda: inst.cloud_organized(src[B], disp.data_ptr(), None, None, xyz.data_ptr()),
}
blocking = {
    "sgm_track 1 frame, 1 round": lambda: track(1, 1),
    "sgm_track 1 frame, 4 rounds": lambda: track(1, 4),
    "sgm_track 8 frames, 4 rounds": lambda: track(B, 4),
}

stream = torch.cuda.ExternalStream(inst.stream)
us = {name: [] for name in list(queued) + list(blocking)}
for _ in range(args.rounds):
    for name, call in queued.items():
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
    if name.startswith("sgm_track_sums"):
        f = 1 if " 1 frame" in name else B
        row["ns_per_source_pixel"] = round(med * 1e3 / (f * W * H), 3)
    print(json.dumps(row))
print(json.dumps({"case": "the tracked batch", "label": args.label, **shape}))
inst.close()
