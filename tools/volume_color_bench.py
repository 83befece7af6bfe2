"""What colour in the TSDF volume costs a call, each coloured call beside its plain twin in the same run (NOTES.md section 39) --
needs an MI355X.

    python tools/volume_color_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label this]

KITTI 1242x375, D = 128, batch 8, device-resident: the disparity maps of a real match of SGM_SynthPair frames and their left images.
The volume of tools/volume_bench.py: 512 x 128 x 512 voxels of 0.1 m (134 MB, and as much again for the colours) in front of the
rig, eight poses advancing 0.5 m along Z.  The plain calls by turns in rounds of their own, then the coloured ones (a plain call timed
between coloured ones would find the 134 MB of its volume pushed out of the caches by their 268 MB, which a library without colour
never does to it):
  sgm_volume_integrate beside sgm_volume_integrate_color (grey, channels 1), for the first frame alone and for the batch, each on
      arrays of its own that see the same calls; the batch with a four-channel image as well;
  sgm_volume_raycast beside sgm_volume_raycast_color, one KITTI-sized view from the first pose, with and without normals;
  sgm_volume_mesh and then sgm_volume_colors on its vertices, queued behind it with its counts.
The method of tools/volume_bench.py: per round and call `warmup` calls, then `calls` calls queued back to back between two HIP
events on the instance's stream; time per call = elapsed / calls.  Median, minimum and maximum over the rounds.  Prints one JSON
line per call and a table.  A library without the coloured entry points (SGM_LIBRARY_PATH pointing at the build of an older commit)
gives the plain rows alone: that is how the plain calls are compared across commits.  --label names the build in the output."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="this")
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
inst = S.SGMInstance(0, batch=B)
assert inst.reset(W, H, S.default_option(D)) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()) and inst.synchronize()
colored = hasattr(inst.lib, "sgm_volume_colors")
rgb = (l.to(torch.int32) * 0x010101).contiguous()               # the grey as r | g << 8 | b << 16

FX, FY, CX, CY, BASELINE = 721.5377, 721.5377, 609.5593, 172.854, 0.54
NX, NY, NZ, VOXEL, TRUNC = 512, 128, 512, 0.1, 0.4
vol = S.volume_spec(NX, NY, NZ, VOXEL, (-0.5 * NX * VOXEL, -0.5 * NY * VOXEL, 2.0), TRUNC, max_weight=64)
NV = NX * NY * NZ
poses = np.zeros((B, 12), np.float32)
poses[:, [0, 4, 8]] = 1.0
poses[:, 11] = -0.5 * np.arange(B)                               # world -> camera of a rig that has advanced 0.5 m per frame
src = {1: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=1), B: S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B)}
view = S.raycast_spec(W, H, FX, FY, CX, CY, 2.0, 53.0, 0.1, 1, 1)

zeros = lambda n, dtype=torch.int32: torch.zeros(n, dtype=dtype, device="cuda")
voxels, voxels_c, colors = zeros(NV), zeros(NV), zeros(NV)
depth, normal, rgba = zeros(W * H, torch.float32), zeros(3 * W * H, torch.float32), zeros(W * H)
counts = zeros(4)

plain = {"sgm_volume_integrate B = 1": lambda: inst.volume_integrate(vol, src[1], poses[:1], disp.data_ptr(), None, None, voxels.data_ptr()),
         "sgm_volume_integrate B = 8": lambda: inst.volume_integrate(vol, src[B], poses, disp.data_ptr(), None, None, voxels.data_ptr())}
tinted = {}
if colored:
    tinted.update({
        "sgm_volume_integrate_color B = 1, grey": lambda: inst.volume_integrate_color(vol, src[1], poses[:1], disp.data_ptr(), None, None, l.data_ptr(), 1,
                                                                                      voxels_c.data_ptr(), colors.data_ptr()),
        "sgm_volume_integrate_color B = 8, grey": lambda: inst.volume_integrate_color(vol, src[B], poses, disp.data_ptr(), None, None, l.data_ptr(), 1,
                                                                                      voxels_c.data_ptr(), colors.data_ptr()),
        "sgm_volume_integrate_color B = 8, four channels": lambda: inst.volume_integrate_color(vol, src[B], poses, disp.data_ptr(), None, None,
                                                                                               rgb.data_ptr(), 4, voxels_c.data_ptr(), colors.data_ptr())})

stream = torch.cuda.ExternalStream(inst.stream)


def measure(calls):
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
    return us


# the plain calls in rounds of their own, so that they meet the caches a library without colour leaves them; then the coloured ones
us = measure(plain)
us.update(measure(tinted))
# the volume as one batch leaves it, for the calls that read it
voxels.zero_(); voxels_c.zero_(); colors.zero_()
assert plain["sgm_volume_integrate B = 8"]() and inst.synchronize()
if colored:
    assert tinted["sgm_volume_integrate_color B = 8, grey"]() and inst.synchronize()
    assert torch.equal(voxels, voxels_c)
assert inst.volume_mesh(vol, voxels.data_ptr(), 1, None, 0, None, 0, counts.data_ptr()) and inst.synchronize()
nv, nt = (int(x) for x in counts.cpu().numpy().view(np.uint32)[:2])
assert nv > 0 and nt > 0
vertices, triangles, vertex_rgba = zeros(4 * nv, torch.float32), zeros(4 * nt), zeros(nv)
mesh = lambda: inst.volume_mesh(vol, voxels.data_ptr(), 1, vertices.data_ptr(), nv, triangles.data_ptr(), nt, counts.data_ptr())
readers = {"sgm_volume_raycast": lambda: inst.volume_raycast(vol, view, poses[:1], voxels.data_ptr(), depth.data_ptr(), normal.data_ptr()),
           "sgm_volume_raycast, depth alone": lambda: inst.volume_raycast(vol, view, poses[:1], voxels.data_ptr(), depth.data_ptr(), None),
           "sgm_volume_mesh": mesh}
tinted = {}
if colored:
    tinted.update({
        "sgm_volume_raycast_color": lambda: inst.volume_raycast_color(vol, view, poses[:1], voxels.data_ptr(), colors.data_ptr(), depth.data_ptr(),
                                                                      normal.data_ptr(), rgba.data_ptr()),
        "sgm_volume_raycast_color, depth alone": lambda: inst.volume_raycast_color(vol, view, poses[:1], voxels.data_ptr(), colors.data_ptr(),
                                                                                   depth.data_ptr(), None, rgba.data_ptr()),
        "sgm_volume_mesh + sgm_volume_colors": lambda: mesh() and inst.volume_colors(vol, voxels.data_ptr(), colors.data_ptr(), vertices.data_ptr(), nv,
                                                                                     counts.data_ptr(), 8, vertex_rgba.data_ptr()),
        "sgm_volume_colors": lambda: inst.volume_colors(vol, voxels.data_ptr(), colors.data_ptr(), vertices.data_ptr(), nv, counts.data_ptr(), 8,
                                                        vertex_rgba.data_ptr())})
us.update(measure(readers))
us.update(measure(tinted))
hits = int(torch.isfinite(depth).sum())
painted = int((rgba != 0).sum()) if colored else 0
facts = {"voxels": NV, "vertices": nv, "triangles": nt, "pixels_of_the_view": W * H, "hits": hits, "coloured_pixels": painted,
         "coloured_voxels": int((colors.view(torch.uint8)[3::4] != 0).sum()) if colored else 0,
         "coloured_vertices": int((vertex_rgba != 0).sum()) if colored else 0}
print(json.dumps({"case": "facts", "label": args.label, **facts}))
for name, t in us.items():
    print(json.dumps({"case": name, "label": args.label, "us_per_call_median": round(statistics.median(t), 2), "min": round(min(t), 2),
                      "max": round(max(t), 2), "rounds": [round(x, 2) for x in t], "calls_per_round": args.calls}))
print("%-52s %10s %10s %10s   (%s: us per call over %d rounds of %d calls)" % ("call", "median", "min", "max", args.label, args.rounds, args.calls))
for name, t in us.items():
    print("%-52s %10.1f %10.1f %10.1f" % (name, statistics.median(t), min(t), max(t)))
inst.close()
