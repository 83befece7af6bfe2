"""What a window of the TSDF volume costs a call, beside a plain device-to-device copy of the same arrays and the integration of one
frame in the same run (NOTES.md section 40) -- needs an MI355X.

    python tools/volume_window_bench.py [--rounds 9] [--calls 20] [--warmup 3] [--label this]

The volume of tools/volume_bench.py: 512 x 128 x 512 voxels of 0.1 m (134 MB, and as much again for the colours), device-resident,
filled with random words.  sgm_volume_window of the whole volume into a second pair of arrays with the shifts (4,0,0), (1,0,0),
(0,4,0), (0,0,8) and (64,16,64), each with and without colours: (1,0,0) leaves the 16-byte load path, the others stay on it.
Beside them hipMemcpyAsync device to device of the same arrays (one array, and two) on the same stream -- the yardstick: a window
reads and writes what the copy does, less what the shift drops -- and sgm_volume_integrate of one KITTI frame, what a step of the
caller's loop pays anyway.  The method of tools/volume_bench.py: per round and call `warmup` calls, then `calls` calls queued back
to back between two HIP events on the instance's stream; time per call = elapsed / calls.  Median, minimum and maximum over the
rounds, and each window's median over the copy's.  The result of (4,0,0) is checked against the arrays sliced by torch.  Prints one
JSON line per call and a table.  --label names the build in the output."""
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
args = ap.parse_args()
W, H, D = 1242, 375, 128
left, right = S.synth_pair(W, H, D, 0x5EED0002)
l, r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
disp = torch.empty((H, W), dtype=torch.float32, device="cuda")
inst = S.SGMInstance(0)
assert inst.reset(W, H, S.default_option(D)) and inst.match_device(l.data_ptr(), r.data_ptr(), disp.data_ptr()) and inst.synchronize()

FX, FY, CX, CY, BASELINE = 721.5377, 721.5377, 609.5593, 172.854, 0.54
NX, NY, NZ, VOXEL, TRUNC = 512, 128, 512, 0.1, 0.4
vol = S.volume_spec(NX, NY, NZ, VOXEL, (-0.5 * NX * VOXEL, -0.5 * NY * VOXEL, 2.0), TRUNC, max_weight=64)
NV = NX * NY * NZ
src = S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=1)
pose = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32)

gen = torch.Generator(device="cuda").manual_seed(40)
rand = lambda: torch.randint(-2 ** 31, 2 ** 31 - 1, (NV,), dtype=torch.int32, device="cuda", generator=gen)
voxels, colors = rand(), rand()
out_voxels, out_colors = torch.zeros_like(voxels), torch.zeros_like(colors)
fused = torch.zeros_like(voxels)
stream = torch.cuda.ExternalStream(inst.stream)
SHIFTS = ((4, 0, 0), (1, 0, 0), (0, 4, 0), (0, 0, 8), (64, 16, 64))


def window(shift, color):
    return lambda: inst.volume_window(vol, shift, (NX, NY, NZ), voxels.data_ptr(), colors.data_ptr() if color else None, out_voxels.data_ptr(),
                                      out_colors.data_ptr() if color else None) is not None


def copy(color):
    def call():
        with torch.cuda.stream(stream):
            out_voxels.copy_(voxels, non_blocking=True)
            if color:
                out_colors.copy_(colors, non_blocking=True)
        return True
    return call


calls = {}
for color in (False, True):
    tail = ", with colours" if color else ""
    calls["device-to-device copy" + tail] = copy(color)
    for shift in SHIFTS:
        calls["sgm_volume_window %s%s" % (shift, tail)] = window(shift, color)
calls["sgm_volume_integrate B = 1"] = lambda: inst.volume_integrate(vol, src, pose, disp.data_ptr(), None, None, fused.data_ptr())

# the result, once: the shift (4,0,0) against the arrays sliced
assert window((4, 0, 0), True)() and inst.synchronize()
for got, want in ((out_voxels, voxels), (out_colors, colors)):
    got, want = got.view(NZ, NY, NX), want.view(NZ, NY, NX)
    assert torch.equal(got[:, :, :NX - 4], want[:, :, 4:]) and int(torch.count_nonzero(got[:, :, NX - 4:])) == 0

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

med = {name: statistics.median(t) for name, t in us.items()}
print(json.dumps({"case": "facts", "label": args.label, "voxels": NV, "bytes_per_array": 4 * NV}))
for name, t in us.items():
    base = med["device-to-device copy, with colours" if name.endswith("with colours") else "device-to-device copy"]
    ratio = round(med[name] / base, 3) if name.startswith("sgm_volume_window") else None
    print(json.dumps({"case": name, "label": args.label, "us_per_call_median": round(med[name], 2), "min": round(min(t), 2), "max": round(max(t), 2),
                      "over_the_copy": ratio, "rounds": [round(x, 2) for x in t], "calls_per_round": args.calls}))
print("%-52s %10s %10s %10s %10s   (%s: us per call over %d rounds of %d calls)" % ("call", "median", "min", "max", "x copy", args.label, args.rounds,
                                                                                  args.calls))
for name, t in us.items():
    base = med["device-to-device copy, with colours" if name.endswith("with colours") else "device-to-device copy"]
    print("%-52s %10.1f %10.1f %10.1f %10s" % (name, med[name], min(t), max(t), "%.2f" % (med[name] / base) if name.startswith("sgm_volume_window") else ""))
inst.close()
