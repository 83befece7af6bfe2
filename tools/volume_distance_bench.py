"""What the distance field of the TSDF volume costs a call, beside the integration of one frame, the mesh and a plain device-to-device
copy of the volume in the same run (NOTES.md section 41) -- needs an MI355X.

    python tools/volume_distance_bench.py [--rounds 9] [--calls 20] [--warmup 3] [--label this] [--radii 8,32,128] [--transform-only]

The volume of tools/volume_bench.py: 512 x 128 x 512 voxels of 0.1 m (134 MB), device-resident, the KITTI batch of 8 fused into it
on the device (eight poses advancing 0.5 m along Z).  sgm_volume_distance at r = 8, 32 and 128 (side 0, unknown 0, min_weight 1), the
same at side 1 and with unknown space as an obstacle at r = 8 (dense sites: what the sparse surface does not show), and
sgm_volume_distance_field, signed and unsigned.  Beside them sgm_volume_integrate of one frame, sgm_volume_mesh, and hipMemcpyAsync
device to device of the volume on the same stream.  The floor a transform is reported against is its traffic: 4 + 2 bytes per voxel
for the x pass and 2 + 2 for each of the other two, 14 bytes per voxel; the field's is 2 + 2 + 4 (2 + 4 unsigned); the copy's 4 + 4.
The method of tools/volume_bench.py: per round and call `warmup` calls, then `calls` calls queued back to back between two HIP
events on the instance's stream; time per call = elapsed / calls.  Median, minimum and maximum over the rounds, the bytes per second
against the floor, and the time per floor byte over the copy's.  The r = 8 result is checked on the device: zero exactly on the sites,
never above r * r, equal bytes from two runs.  Prints one JSON line per call and a table.  --label names the build in the output.  --radii R --transform-only times one radius and
the copy alone: under rocprofv3 --kernel-trace --stats the three kernels of the transform (x pass, y pass, z pass) then show what
each pass takes at that radius."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="this")
ap.add_argument("--radii", default="8,32,128", help="the radii to time (side 0, unknown 0)")
ap.add_argument("--transform-only", action="store_true", help="time nothing but the copy and the radii: for a kernel trace of one radius")
args = ap.parse_args()
RADII = [int(x) for x in args.radii.split(",")]
W, H, D, B = 1242, 375, 128, 8
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
inst = S.SGMInstance(0, batch=B)
assert inst.reset(W, H, S.default_option(D)) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()) and inst.synchronize()

FX, FY, CX, CY, BASELINE = 721.5377, 721.5377, 609.5593, 172.854, 0.54
NX, NY, NZ, VOXEL, TRUNC = 512, 128, 512, 0.1, 0.4
vol = S.volume_spec(NX, NY, NZ, VOXEL, (-0.5 * NX * VOXEL, -0.5 * NY * VOXEL, 2.0), TRUNC, max_weight=64)
NV = NX * NY * NZ
assert S.volume_distance_bytes(vol) == 2 * NV
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src1, src8 = (S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=f) for f in (1, B))
voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")
assert inst.volume_integrate(vol, src8, poses, disp.data_ptr(), None, None, voxels.data_ptr()) and inst.synchronize()
scratch_volume, copied = voxels.clone(), torch.zeros_like(voxels)
out2, in2 = (torch.zeros(NV, dtype=torch.int16, device="cuda") for _ in range(2))
field = torch.zeros(NV, dtype=torch.float32, device="cuda")
counts = torch.zeros(4, dtype=torch.int32, device="cuda")
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, None, 0, None, 0, counts.data_ptr()) and inst.synchronize()
n_vert, n_tri = (int(x) for x in counts.cpu().numpy().view(np.uint32)[:2])
vertices = torch.empty(4 * max(n_vert, 1), dtype=torch.int32, device="cuda")
triangles = torch.empty(4 * max(n_tri, 1), dtype=torch.int32, device="cuda")
stream = torch.cuda.ExternalStream(inst.stream)


def distance(radius, side=0, unknown=0, into=out2):
    spec = S.distance_spec(1, radius, side, unknown)
    return lambda: inst.volume_distance(vol, spec, voxels.data_ptr(), into.data_ptr())


def copy():
    with torch.cuda.stream(stream):
        copied.copy_(voxels, non_blocking=True)
    return True


# the r = 8 result, once: zero exactly on the sites, nothing between r * r and FAR, the same bytes from a second run
observed, negative = (voxels >> 16) != 0, (voxels & 0x8000) != 0     # min_weight 1
occupied = observed & negative
assert distance(8)() and inst.synchronize()
first = out2.clone()
assert torch.equal(first == 0, occupied) and not bool(((first > 64) | (first < -1)).any())
assert distance(8)() and inst.synchronize() and torch.equal(first, out2)
assert distance(8, side=1, into=in2)() and inst.synchronize() and torch.equal(in2 == 0, ~occupied)
facts = {"case": "facts", "label": args.label, "voxels": NV, "observed": int(observed.sum()), "occupied": int(occupied.sum()),
         "within_r8": int((first != -1).sum()), "mesh_vertices": n_vert, "mesh_triangles": n_tri, "floor_bytes_transform": 14 * NV}
for radius in (x for x in RADII if x != 8):
    assert distance(radius)() and inst.synchronize()
    facts["within_r%d" % radius] = int((out2 != -1).sum())
del first

# name -> (the call, its floor in bytes per voxel or None)
calls = {"hipMemcpyAsync of the volume, device to device": (copy, 8)}
for radius in RADII:
    calls["sgm_volume_distance r = %d" % radius] = (distance(radius), 14)
calls["sgm_volume_distance r = 8, side 1"] = (distance(8, side=1, into=in2), 14)
calls["sgm_volume_distance r = 8, unknown 1"] = (distance(8, unknown=1), 14)
calls["sgm_volume_distance r = 8 (again, for the field)"] = (distance(8), 14)
calls["sgm_volume_distance_field signed"] = (lambda: inst.volume_distance_field(vol, out2.data_ptr(), in2.data_ptr(), field.data_ptr()), 8)
calls["sgm_volume_distance_field unsigned"] = (lambda: inst.volume_distance_field(vol, out2.data_ptr(), None, field.data_ptr()), 6)
calls["sgm_volume_integrate B = 1"] = (lambda: inst.volume_integrate(vol, src1, poses[:1], disp.data_ptr(), None, None, scratch_volume.data_ptr()), None)
calls["sgm_volume_mesh"] = (lambda: inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), n_vert, triangles.data_ptr(), n_tri,
                                                     counts.data_ptr()), None)

if args.transform_only:
    calls = {name: c for name, c in calls.items() if name.startswith("hipMemcpyAsync") or name in ["sgm_volume_distance r = %d" % x for x in RADII]}
us = {name: [] for name in calls}
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

med = {name: statistics.median(t) for name, t in us.items()}
copy_us_per_byte = med["hipMemcpyAsync of the volume, device to device"] / (8 * NV)
print(json.dumps(facts))
rows = []
for name, t in us.items():
    floor = calls[name][1]
    gbs = round(floor * NV / med[name] / 1e3, 1) if floor else None          # bytes / us / 1e3 = GB/s
    per_byte = round(med[name] / (floor * NV) / copy_us_per_byte, 2) if floor else None
    rows.append((name, gbs, per_byte))
    print(json.dumps({"case": name, "label": args.label, "us_per_call_median": round(med[name], 2), "min": round(min(t), 2), "max": round(max(t), 2),
                      "floor_bytes": floor * NV if floor else None, "floor_GBps": gbs, "time_per_floor_byte_over_the_copys": per_byte,
                      "rounds": [round(x, 2) for x in t], "calls_per_round": args.calls}))
print("%-52s %10s %10s %10s %10s %8s   (%s: us per call over %d rounds of %d calls; GB/s of the floor; time per floor byte over the copy's)"
      % ("call", "median", "min", "max", "GB/s", "x copy", args.label, args.rounds, args.calls))
for name, gbs, per_byte in rows:
    t = us[name]
    print("%-52s %10.1f %10.1f %10.1f %10s %8s" % (name, med[name], min(t), max(t), "" if gbs is None else "%.1f" % gbs, "" if per_byte is None else "%.2f" % per_byte))
inst.close()
