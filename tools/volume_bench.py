"""What fusing depth into a TSDF volume costs a call (NOTES.md section 31) -- needs an MI355X.

    python tools/volume_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label plain]

KITTI 1242x375, D = 128, batch 8, device-resident: the disparity maps of a real match of SGM_SynthPair frames.  A volume of
512 x 128 x 512 voxels of 0.1 m (134 MB) in front of the rig, eight poses advancing 0.5 m along Z.  By turns on that map:
sgm_volume_integrate of the first frame alone (B = 1) and of the batch (B = 8), sgm_volume_points on the result, and as yardsticks
sgm_cloud_organized, sgm_cloud_points and the temporal filter (sgm_temporal_filter, one step of eight streams).  The method of
section 29: per round and call `warmup` calls, then `calls` calls queued back to back between two HIP events on the instance's
stream; time per call = elapsed / calls.  Median, minimum and maximum over the rounds.  Beside the integration: the voxels a call
updates and stores, the bytes it moves (every word read once, the stored ones written once) and the rate that is, against one read
plus one write of the updated voxels alone.  Prints one JSON line per call and the match's own time per batch.  --label names the
build in the output (SGM_LIBRARY_PATH may point at the library of another commit)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="plain")
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

FX, FY, CX, CY, BASELINE = 721.5377, 721.5377, 609.5593, 172.854, 0.54
NX, NY, NZ, VOXEL, TRUNC = 512, 128, 512, 0.1, 0.4
vol = S.volume_spec(NX, NY, NZ, VOXEL, (-0.5 * NX * VOXEL, -0.5 * NY * VOXEL, 2.0), TRUNC, max_weight=64)
NV = NX * NY * NZ
assert S.volume_bytes(vol) == 4 * NV
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src = {1: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=1), B: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B)}

voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")
count = torch.zeros(4, dtype=torch.int32, device="cuda")


def integrate(frames):
    return inst.volume_integrate(vol, src[frames], poses[:frames], disp.data_ptr(), None, None, voxels.data_ptr())


# what one call from the empty volume updates and stores (a lane stores its four voxels when one of them was updated)
traffic = {}
for frames in (1, B):
    voxels.zero_()
    assert integrate(frames) and inst.synchronize()
    seen = (voxels.view(-1, 4) >> 16) != 0
    traffic[frames] = (int(seen.sum()), 4 * int(seen.any(dim=1).sum()))
assert inst.volume_points(vol, voxels.data_ptr(), 1, None, 0, count.data_ptr()) and inst.synchronize()
crossings = int(count.cpu().numpy().view(np.uint32)[0])
points = torch.empty(4 * max(crossings, 1), dtype=torch.float32, device="cuda")

xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")
cloud_pts = torch.empty(4 * N, dtype=torch.float32, device="cuda")
offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
filtered = disp.clone()
hist_value = torch.zeros(N, dtype=torch.float32, device="cuda")
hist_bits = torch.zeros(N, dtype=torch.uint8, device="cuda")
tspec = S.temporal_spec()
calls = {
    "sgm_volume_integrate B = 1": lambda: integrate(1),
    "sgm_volume_integrate B = 8": lambda: integrate(B),
    "sgm_volume_points": lambda: inst.volume_points(vol, voxels.data_ptr(), 1, points.data_ptr(), crossings, count.data_ptr()),
    "sgm_cloud_organized": lambda: inst.cloud_organized(src[B], disp.data_ptr(), None, None, xyz.data_ptr()),
    "sgm_cloud_points": lambda: inst.cloud_points(src[B], disp.data_ptr(), None, None, cloud_pts.data_ptr(), offsets.data_ptr()),
    "sgm_temporal_filter": lambda: inst.temporal_filter(tspec, B, 1, W * H, filtered.data_ptr(), None, hist_value.data_ptr(), hist_bits.data_ptr()),
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
assert int(count.cpu().numpy().view(np.uint32)[0]) > 0 and crossings > 0
finite = int(torch.isfinite(disp).sum())
print(json.dumps({"case": "match", "label": args.label, "ms_per_batch_median": round(statistics.median(match_ms), 4), "min": round(min(match_ms), 4),
                  "max": round(max(match_ms), 4), "pixels": N, "finite_disparities": finite}))
for name in calls:
    med = statistics.median(us[name])
    row = {"case": name, "label": args.label, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
           "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls,
           "share_of_match": round(med * 1e-3 / statistics.median(match_ms), 4)}
    if name.startswith("sgm_volume_integrate"):
        updated, stored = traffic[1 if name.endswith("1") else B]
        moved = 4 * NV + 4 * stored
        row.update({"voxels": NV, "voxels_updated": updated, "voxels_stored": stored, "bytes_moved": moved,
                    "GB_per_s_moved": round(moved / (med * 1e-6) / 1e9, 1), "bytes_read_plus_write_of_the_updated": 8 * updated,
                    "GB_per_s_of_the_updated_alone": round(8 * updated / (med * 1e-6) / 1e9, 1)})
    if name == "sgm_volume_points":
        moved = 2 * 4 * NV + 16 * crossings                      # count and emit read every word once each; the neighbours hit a cache
        row.update({"voxels": NV, "crossings_after_one_batch": crossings, "bytes_moved_at_least": moved,
                    "GB_per_s_at_least": round(moved / (med * 1e-6) / 1e9, 1)})
    print(json.dumps(row))
inst.close()
