"""What the connected components of the TSDF volume cost a call, beside the distance field, the mesh and a plain device-to-device
copy of the volume in the same run (NOTES.md section 44) -- needs an MI355X.

    python tools/volume_components_bench.py [--rounds 9] [--calls 10] [--warmup 2] [--label this] [--only NAME-PART]

The volume of tools/volume_distance_bench.py: 512 x 128 x 512 voxels of 0.1 m (134 MB), device-resident, the KITTI batch of 8 fused
into it on the device.  sgm_volume_components on the occupied set at 6 and at 26, on the free set (most of the volume: one component
of millions of voxels), on the occupied set with the plane sgm_plane_fit found in the surface points excluded, each with room for
every record and with capacity 0 (labels and counts alone); sgm_volume_component_of on the mesh's vertices.  Beside them
sgm_volume_distance at r = 8, sgm_volume_mesh and hipMemcpyAsync device to device of the volume on the same stream.  The yardstick
is that copy: the call must read 4 bytes and write 4 bytes per voxel at least once, so its floor is the copy's traffic, and the
column "x copy" is the time of a call over the copy's.  The method of tools/volume_bench.py: per round and call `warmup` calls, then
`calls` calls queued back to back between two HIP events on the instance's stream; time per call = elapsed / calls.  Median, minimum
and maximum over the rounds.  The result is checked on the device: labels non-zero exactly on the set (min_voxels 1), equal bytes
from two runs, the records' voxels summing to the set.  The global unions are counted here from the labels of a run and the 64 x 8 x 8 tile of the
source, by the border launch's own rule restated on whole arrays (border_unions): one per pair of neighbours in different tiles that
no voxel to the left implies.  A lower bound stands beside it: a component that lies in t tiles holds at least t tile-local
components, and joining them takes t - 1 unions at the least.  Prints one JSON line
per call and a table.  --only: time nothing but the copy and the calls whose name contains the text (for a kernel trace of one call
under rocprofv3 --kernel-trace --stats, which then shows each launch's share)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="this")
ap.add_argument("--only", default="")
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
assert S.volume_components_bytes(vol) == 4 * NV
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src8 = S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B)
voxels = torch.zeros(NV, dtype=torch.int32, device="cuda")
assert inst.volume_integrate(vol, src8, poses, disp.data_ptr(), None, None, voxels.data_ptr()) and inst.synchronize()
copied = torch.zeros_like(voxels)
labels = torch.zeros(NV, dtype=torch.int32, device="cuda")
out2 = torch.zeros(NV, dtype=torch.int16, device="cuda")
counts = torch.zeros(4, dtype=torch.int32, device="cuda")
mesh_counts = torch.zeros(4, dtype=torch.int32, device="cuda")
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, None, 0, None, 0, mesh_counts.data_ptr()) and inst.synchronize()
n_vert, n_tri = (int(x) for x in mesh_counts.cpu().numpy().view(np.uint32)[:2])
vertices = torch.empty(4 * max(n_vert, 1), dtype=torch.int32, device="cuda")
triangles = torch.empty(4 * max(n_tri, 1), dtype=torch.int32, device="cuda")
index = torch.zeros(max(n_vert, 1), dtype=torch.int32, device="cuda")
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), n_vert, triangles.data_ptr(), n_tri, mesh_counts.data_ptr()) and inst.synchronize()
stream = torch.cuda.ExternalStream(inst.stream)

# the floor: the plane of the surface points, its normal turned towards the camera's up (-y); what stands above it by 0.3 m stays
fit = inst.plane_fit(S.plane_spec(1024, 0.1, 20.0, seed=1, axis=(0.0, -1.0, 0.0), min_cos=0.8, iterations=4, min_inliers=100, min_pivot=1e-9),
                     vertices.data_ptr(), n_vert, mesh_counts.data_ptr(), None)
floor = fit[0] if fit is not None and fit[1]["status"] == 0 else None
CLEARANCE = 0.3


def run(comp, capacity, objects):
    return lambda: inst.volume_components(vol, comp, voxels.data_ptr(), labels.data_ptr(), objects.data_ptr() if capacity else None, capacity,
                                          counts.data_ptr())


def read_counts():
    return tuple(int(x) for x in counts.cpu().numpy().view(np.uint32)[:2])


cases = {"occupied, 6": S.component_spec(1, 0, 0, 6), "occupied, 26": S.component_spec(1, 0, 0, 26), "free, 6": S.component_spec(1, 1, 0, 6)}
if floor is not None:
    cases["occupied, 26, floor excluded"] = S.component_spec(1, 0, 0, 26, 1, [floor], [CLEARANCE])
observed, negative = (voxels >> 16) != 0, (voxels & 0x8000) != 0     # min_weight 1
members = {"occupied, 6": observed & negative, "occupied, 26": observed & negative, "free, 6": observed & ~negative}
facts = {"case": "facts", "label": args.label, "voxels": NV, "observed": int(observed.sum()), "occupied": int((observed & negative).sum()),
         "mesh_vertices": n_vert, "floor": None if floor is None else {"normal": [round(float(x), 4) for x in floor["normal"]],
                                                                       "offset": round(float(floor["offset"]), 4), "clearance": CLEARANCE}}
TX, TY, TZ = 64, 8, 8


def border_unions(inside, connectivity):
    """(the unions the border launch makes on the set `inside` (bool [NZ][NY][NX]), the voxels of the set it looks at): its own
    rule restated on whole arrays -- a pair of neighbours, both in the set, in different tiles, the earlier one reached by an
    offset below (0, 0, 0), unless the pair one voxel to the left (a straight pair) or the straight pair of this or of the far
    column (a diagonal one) implies it.  Every one is a call of the union; some find their two roots joined already."""
    M = torch.zeros((NZ + 2, NY + 2, NX + 2), dtype=torch.bool, device="cuda")
    M[1:-1, 1:-1, 1:-1] = inside
    at = lambda dx, dy, dz: M[1 + dz:1 + dz + NZ, 1 + dy:1 + dy + NY, 1 + dx:1 + dx + NX]      # in(p + d), nothing outside the grid
    X, Y, Z = torch.arange(NX, device="cuda")[None, None, :], torch.arange(NY, device="cuda")[None, :, None], torch.arange(NZ, device="cuda")[:, None, None]
    face = (X % TX == 0) | (Y % TY == 0) | (Z % TZ == 0)
    if connectivity == 26:
        face = face | (X % TX == TX - 1) | (Y % TY == TY - 1)
    total = 0
    for o in range(13):
        dx, dy, dz = o % 3 - 1, o // 3 % 3 - 1, o // 9 - 1
        if connectivity == 6 and (dx != 0) + (dy != 0) + (dz != 0) != 1:
            continue
        other = ((X + dx) // TX != X // TX) | ((Y + dy) // TY != Y // TY) | ((Z + dz) // TZ != Z // TZ)
        link = inside & at(dx, dy, dz) & other
        if dy != 0 or dz != 0:
            if dx == 0:
                link = link & ~(at(-1, 0, 0) & at(-1, dy, dz))
            elif dx < 0:
                link = link & ~(at(0, dy, dz) | at(-1, 0, 0))
            else:
                link = link & ~(at(0, dy, dz) | at(1, 0, 0))
        total += int(link.sum())
    return total, int((inside & face).sum())


objects, calls = {}, {}
for name, comp in cases.items():
    assert run(comp, 0, None)() and inst.synchronize()
    C, everything = read_counts()
    obj = torch.zeros(12 * max(C, 1), dtype=torch.int32, device="cuda")
    objects[name] = obj
    assert run(comp, C, obj)() and inst.synchronize() and read_counts() == (C, everything)
    first = labels.clone()
    rec = np.frombuffer(obj.cpu().numpy().tobytes(), S.COMPONENT_DTYPE)[:C]
    if name in members:
        assert torch.equal(first != 0, members[name])
    assert int(rec["voxels"].astype(np.int64).sum()) == int((first != 0).sum()) and np.all(np.diff(rec["first"].astype(np.int64)) > 0)
    assert run(comp, C, obj)() and inst.synchronize() and torch.equal(first, labels)
    assert np.frombuffer(obj.cpu().numpy().tobytes(), S.COMPONENT_DTYPE)[:C].tobytes() == rec.tobytes()
    # pairs of (tile, label) = the tile-local components at the least; the voxels on tile faces: what the border launch looks at
    lab = first.view(NZ, NY, NX)
    tile_of = ((torch.arange(NZ, device="cuda") // TZ)[:, None, None] * (NY // TY) + (torch.arange(NY, device="cuda") // TY)[None, :, None]) * (NX // TX) + \
        (torch.arange(NX, device="cuda") // TX)[None, None, :]
    keys = (tile_of.to(torch.int64) << 32 | (lab.to(torch.int64) & 0xFFFFFFFF))[lab != 0]
    facts[name] = {"components": C, "largest": int(rec["voxels"].max()) if C else 0, "in_the_set": int((first != 0).sum()),
                   "tile_label_pairs": int(torch.unique(keys).numel()), "tiles": (NX // TX) * (NY // TY) * (NZ // TZ)}
    # every pair of tile-local components adds one union at the least: pairs - components is the least number of global unions
    facts[name]["global_unions_at_least"] = facts[name]["tile_label_pairs"] - C
    facts[name]["global_unions"], facts[name]["face_voxels_in_the_set"] = border_unions(lab != 0, 26 if ", 26" in name else 6)
    calls["sgm_volume_components " + name] = run(comp, C, obj)
    calls["sgm_volume_components " + name + ", capacity 0"] = run(comp, 0, None)
    del first, lab, keys
C26 = facts["occupied, 26"]["components"]
assert run(cases["occupied, 26"], C26, objects["occupied, 26"])() and inst.synchronize()
calls["sgm_volume_component_of the mesh's vertices"] = lambda: inst.volume_component_of(
    vol, labels.data_ptr(), objects["occupied, 26"].data_ptr(), C26, counts.data_ptr(), vertices.data_ptr(), n_vert, mesh_counts.data_ptr(), 8, index.data_ptr())
assert calls["sgm_volume_component_of the mesh's vertices"]() and inst.synchronize()
facts["vertices_with_an_object"] = int((index != 0).sum())


def copy():
    with torch.cuda.stream(stream):
        copied.copy_(voxels, non_blocking=True)
    return True


dist = S.distance_spec(1, 8, 0, 0)
timed = {"hipMemcpyAsync of the volume, device to device": copy}
# (component_of reads the labels of "occupied, 26": it is timed first, before the other cases write the array)
timed["sgm_volume_component_of the mesh's vertices"] = calls.pop("sgm_volume_component_of the mesh's vertices")
timed.update(calls)
timed["sgm_volume_distance r = 8"] = lambda: inst.volume_distance(vol, dist, voxels.data_ptr(), out2.data_ptr())
timed["sgm_volume_mesh"] = lambda: inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), n_vert, triangles.data_ptr(), n_tri, mesh_counts.data_ptr())
if args.only:
    timed = {name: c for name, c in timed.items() if name.startswith("hipMemcpyAsync") or args.only in name}
us = {name: [] for name in timed}
for _ in range(args.rounds):
    for name, call in timed.items():
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
copy_us = med["hipMemcpyAsync of the volume, device to device"]
print(json.dumps(facts))
for name, t in us.items():
    print(json.dumps({"case": name, "label": args.label, "us_per_call_median": round(med[name], 2), "min": round(min(t), 2), "max": round(max(t), 2),
                      "over_the_copy": round(med[name] / copy_us, 2), "rounds": [round(x, 2) for x in t], "calls_per_round": args.calls}))
print("%-60s %10s %10s %10s %8s   (%s: us per call over %d rounds of %d calls; the copy moves 8 bytes per voxel: %.1f GB/s)"
      % ("call", "median", "min", "max", "x copy", args.label, args.rounds, args.calls, 8 * NV / copy_us / 1e3))
for name, t in us.items():
    print("%-60s %10.1f %10.1f %10.1f %8.2f" % (name, med[name], min(t), max(t), med[name] / copy_us))
inst.close()
