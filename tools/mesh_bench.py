"""What the volume's mesh costs a call (NOTES.md section 37) -- needs an MI355X.

    python tools/mesh_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label head]

The volume of tools/volume_bench.py (NOTES.md sections 31 and 34): KITTI 1242x375, D = 128, batch 8, the disparity maps of a real
match of SGM_SynthPair frames fused into 512 x 128 x 512 voxels of 0.1 m (134 MB), eight poses advancing 0.5 m along Z.  By turns
on that volume: sgm_volume_mesh counts-only (both capacities 0), sgm_volume_mesh in full (arrays of exactly the counts), and beside
them sgm_volume_points counts-only and in full.  The method of section 29: per round and call `warmup` calls, then `calls` calls
queued back to back between two HIP events on the instance's stream; time per call = elapsed / calls.  Median, minimum and maximum
over the rounds.  Prints one JSON line per call with the counts, and checks the mesh once: every triangle index is below the vertex
count and the axis vertices are the surface points.  --label names the build in the output."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="head")
args = ap.parse_args()
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
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")
assert inst.volume_integrate(vol, S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B), poses, disp.data_ptr(), None, None,
                             voxels.data_ptr())
counts = torch.zeros(4, dtype=torch.int32, device="cuda")
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, None, 0, None, 0, counts.data_ptr()) and inst.synchronize()
n_vert, n_tri = (int(x) for x in counts.cpu().numpy().view(np.uint32)[:2])
assert inst.volume_points(vol, voxels.data_ptr(), 1, None, 0, counts.data_ptr() + 8) and inst.synchronize()
crossings = int(counts.cpu().numpy().view(np.uint32)[2])
vertices = torch.empty(4 * max(n_vert, 1), dtype=torch.int32, device="cuda")
triangles = torch.empty(4 * max(n_tri, 1), dtype=torch.int32, device="cuda")
points = torch.empty(4 * max(crossings, 1), dtype=torch.int32, device="cuda")

# the mesh once, checked: indices inside the vertex list, ids ascending, the axis vertices are the surface points
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), n_vert, triangles.data_ptr(), n_tri, counts.data_ptr())
assert inst.volume_points(vol, voxels.data_ptr(), 1, points.data_ptr(), crossings, counts.data_ptr() + 8) and inst.synchronize()
vert = vertices.cpu().numpy().view(S.MESH_VERTEX_DTYPE)[:n_vert]
tri = triangles.cpu().numpy().view(S.MESH_TRIANGLE_DTYPE)[:n_tri]
pts = points.cpu().numpy().view(S.SURFACE_DTYPE)[:crossings]
assert n_tri > 0 and int(tri["v"].max()) < n_vert and np.all(np.diff(vert["id"].astype(np.int64)) > 0)
axis = vert[(vert["id"] & 7) < 3]
assert len(axis) == crossings and all(axis[n].tobytes() == pts[n].tobytes() for n in "xyz")
used = len(np.unique(tri["v"]))

calls = {
    "sgm_volume_mesh counts only": lambda: inst.volume_mesh(vol, voxels.data_ptr(), 1, None, 0, None, 0, counts.data_ptr()),
    "sgm_volume_mesh": lambda: inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), n_vert, triangles.data_ptr(), n_tri, counts.data_ptr()),
    "sgm_volume_points count only": lambda: inst.volume_points(vol, voxels.data_ptr(), 1, None, 0, counts.data_ptr() + 8),
    "sgm_volume_points": lambda: inst.volume_points(vol, voxels.data_ptr(), 1, points.data_ptr(), crossings, counts.data_ptr() + 8),
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
    print(json.dumps({"case": name, "label": args.label, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2),
                      "max": round(max(us[name]), 2), "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls, "voxels": NV,
                      "vertices": n_vert, "vertices_used_by_a_triangle": used, "triangles": n_tri, "surface_points": crossings,
                      "scratch_bytes": 16 * ((NV + 2047) // 2048)}))
inst.close()
