"""What rendering the TSDF volume into a view costs a call (NOTES.md section 34) -- needs an MI355X.

    python tools/raycast_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label tile+skip]

The set-up of tools/volume_bench.py: KITTI 1242x375, D = 128, batch 8, device-resident, the disparity maps of a real match of
SGM_SynthPair frames fused (sgm_volume_integrate, B = 8) into 512 x 128 x 512 voxels of 0.1 m (134 MB) in front of the rig, eight
poses advancing 0.5 m along Z.  By turns on that volume: sgm_volume_raycast of the 1242x375 view of frame 0 and of all eight poses,
with and without normals, marched from 0.5 m to 55 m in steps of 0.2 m (half the truncation distance: 273 samples where nothing is
met), and as yardsticks sgm_volume_integrate B = 1, sgm_volume_points and sgm_cloud_organized.  The method of section 29: per round
and call `warmup` calls, then `calls` calls queued back to back between two HIP events on the instance's stream; time per call =
elapsed / calls.  Median, minimum and maximum over the rounds.  Beside the render: the pixels that meet the surface and the samples
per pixel the contract's march takes (from the depth map: up to the hit, or all of them), i.e. without the box skip.  Prints one JSON
line per call.  --label names the build in the output (SGM_LIBRARY_PATH may point at the library of another commit)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="tile+skip")
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
NV = NX * NY * NZ
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src = {f: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=f) for f in (1, B)}
view = {f: S.raycast_spec(W, H, FX, FY, CX, CY, Z_MIN, Z_MAX, STEP, 1, frames=f) for f in (1, B)}

voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")
scratch_voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")             # what the integration yardstick writes
count = torch.zeros(4, dtype=torch.int32, device="cuda")
assert inst.volume_integrate(vol, src[B], poses, disp.data_ptr(), None, None, voxels.data_ptr())
assert inst.volume_points(vol, voxels.data_ptr(), 1, None, 0, count.data_ptr()) and inst.synchronize()
crossings = int(count.cpu().numpy().view(np.uint32)[0])
points = torch.empty(4 * max(crossings, 1), dtype=torch.float32, device="cuda")
depth = torch.empty(N, dtype=torch.float32, device="cuda")
normal = torch.empty(3 * N, dtype=torch.float32, device="cuda")
xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")


def render(frames, normals):
    return inst.volume_raycast(vol, view[frames], poses[:frames], voxels.data_ptr(), depth.data_ptr(), normal.data_ptr() if normals else None)


# what the march of the contract takes per pixel, from the depth maps of the eight views
assert render(B, True) and inst.synchronize()
z = depth.cpu().numpy().astype(np.float64)
hit = np.isfinite(z)
total = int(np.floor((Z_MAX - Z_MIN) / STEP)) + 1
samples = np.where(hit, np.ceil((np.where(hit, z, 0.0) - Z_MIN) / STEP) + 1, total)
with_normal = int(torch.isfinite(normal.view(-1, 3)[:, 0]).sum())
shape = {}
for f in (1, B):
    sel = slice(0, f * W * H)
    shape[f] = {"pixels": f * W * H, "pixels_hit": int(hit[sel].sum()), "samples_per_pixel_without_skip": round(float(samples[sel].mean()), 1),
                "samples_per_pixel_nothing_met": total, "mean_hit_depth_m": round(float(z[sel][hit[sel]].mean()), 2)}

calls = {
    "sgm_volume_raycast 1 view, depth": lambda: render(1, False),
    "sgm_volume_raycast 1 view, depth + normals": lambda: render(1, True),
    "sgm_volume_raycast 8 views, depth": lambda: render(B, False),
    "sgm_volume_raycast 8 views, depth + normals": lambda: render(B, True),
    "sgm_volume_integrate B = 1": lambda: inst.volume_integrate(vol, src[1], poses[:1], disp.data_ptr(), None, None, scratch_voxels.data_ptr()),
    "sgm_volume_points": lambda: inst.volume_points(vol, voxels.data_ptr(), 1, points.data_ptr(), crossings, count.data_ptr()),
    "sgm_cloud_organized": lambda: inst.cloud_organized(src[B], disp.data_ptr(), None, None, xyz.data_ptr()),
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
for name in calls:
    med = statistics.median(us[name])
    row = {"case": name, "label": args.label, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
           "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls}
    if name.startswith("sgm_volume_raycast"):
        f = 1 if " 1 view" in name else B
        row.update(shape[f])
        row["ns_per_pixel"] = round(med * 1e3 / (f * W * H), 3)
        # one word per sample, 16 for the two trilinear values of a hit, 48 more for its normal
        loads = shape[f]["samples_per_pixel_without_skip"] + (16 + (48 if "normals" in name else 0)) * shape[f]["pixels_hit"] / shape[f]["pixels"]
        row["loads_per_pixel_without_skip"] = round(loads, 1)
        if f == B:
            row["pixels_with_a_normal"] = with_normal
    print(json.dumps(row))
inst.close()
