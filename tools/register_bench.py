"""What registering depth to another camera costs a call (NOTES.md section 29) -- needs an MI355X.

    python tools/register_bench.py [--rounds 9] [--calls 40] [--warmup 5] [--label plain]

KITTI 1242x375, D = 128, batch 8, device-resident: the disparity maps of a real match of SGM_SynthPair frames.  By turns on that map:
sgm_register_depth at splat 1 and 2 into an identity target (the source's own pinhole) and into the raw camera of the SMALL model of
tests/rectify_ref.py (sgm_register_spec_raw), sgm_register_gather of a u16 map, and as yardsticks sgm_cloud_organized and
sgm_cloud_points.  Per round and call: `warmup` calls, then `calls` calls queued back to back between two HIP events on the
instance's stream; time per call = elapsed / calls.  Median, minimum and maximum over the rounds.  Beside every registration: the
atomic candidates a call issues (counted by the restatement tests/register_ref.py on the same map) and the byte rate they imply, 8 B
each, over the whole call (clear and resolve included: a lower bound of the scatter's own rate).  Prints one JSON line per call and
the match's own time per batch.  --label names the build in the output (SGM_LIBRARY_PATH may point at the
library of another commit)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import soc_project_stereo_matching_amd as S
import cloud_ref as CR, rectify_ref as RR, register_ref as GR

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
K, dist, R, Knew = RR.model(RR.SMALL, W, H)
sources = {"identity": CR.spec(W, H, fx=FX, fy=FY, cx=CX, cy=CY, baseline=BASELINE, frames=B),
           "raw SMALL": CR.spec(W, H, fx=Knew[0, 0], fy=Knew[1, 1], cx=Knew[0, 2], cy=Knew[1, 2], baseline=BASELINE, frames=B)}
targets = {"identity": lambda splat: GR.spec(W, H, FX, FY, CX, CY, splat=splat), "raw SMALL": lambda splat: GR.spec_raw(K, dist, R, W, H, splat)}


def c_source(s):
    return S.cloud_spec(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.baseline, s.doffs, frames=s.frames)


def c_target(t):
    return S.register_spec(t.width, t.height, t.fx, t.fy, t.cx, t.cy, t.dist, t.R, t.t, t.z_min, t.z_max, t.splat)


def count(host_disp, s, t):
    """(admitted candidates, target pixels they cover) by the restatement's projection"""
    ok, _, u, v = GR.project(host_disp, s, t)
    votes, hit = 0, np.zeros((B, t.height * t.width), bool)
    for uf, vf in GR.candidates(u, v, t.splat):
        with np.errstate(all="ignore"):
            adm = ok & (0 <= uf) & (uf < np.float32(t.width)) & (0 <= vf) & (vf < np.float32(t.height))
        hit[np.nonzero(adm)[0], vf[adm].astype(np.int64) * t.width + uf[adm].astype(np.int64)] = True
        votes += int(adm.sum())
    return votes, int(hit.sum())


depth = torch.empty(N, dtype=torch.float32, device="cuda")
source = torch.empty(N, dtype=torch.int32, device="cuda")
side = torch.zeros(N, dtype=torch.int16, device="cuda")
side_out = torch.empty(N, dtype=torch.int16, device="cuda")
xyz = torch.empty(3 * N, dtype=torch.float32, device="cuda")
points = torch.empty(4 * N, dtype=torch.float32, device="cuda")
offsets = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
host_disp = disp.cpu().numpy()
calls, votes, landed = {}, {}, {}
for where in ("identity", "raw SMALL"):
    for splat in (1, 2):
        name = f"sgm_register_depth {where} splat {splat}"
        cs, ct = c_source(sources[where]), c_target(targets[where](splat))
        calls[name] = lambda cs=cs, ct=ct: inst.register_depth(cs, ct, disp.data_ptr(), None, None, depth.data_ptr(), source.data_ptr())
        votes[name], landed[name] = count(host_disp, sources[where], targets[where](splat))
cs, ct = c_source(sources["raw SMALL"]), c_target(targets["raw SMALL"](2))
calls["sgm_register_gather u16"] = lambda: inst.register_gather(cs, ct, source.data_ptr(), side.data_ptr(), side_out.data_ptr(), np.uint16, 0)
cloud = S.cloud_spec(W, H, FX, FY, CX, CY, BASELINE, 0.0, frames=B)
calls["sgm_cloud_organized"] = lambda: inst.cloud_organized(cloud, disp.data_ptr(), None, None, xyz.data_ptr())
calls["sgm_cloud_points"] = lambda: inst.cloud_points(cloud, disp.data_ptr(), None, None, points.data_ptr(), offsets.data_ptr())

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
# the last registration timed is what `source` and `depth` hold: the device agrees with the restatement that counted the votes
last = [n for n in calls if n.startswith("sgm_register_depth")][-1]
assert int((source.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).sum()) == landed[last]
finite = int(torch.isfinite(disp).sum())
print(json.dumps({"case": "match", "label": args.label, "ms_per_batch_median": round(statistics.median(match_ms), 4), "min": round(min(match_ms), 4),
                  "max": round(max(match_ms), 4), "pixels": N, "finite_disparities": finite}))
for name in calls:
    med = statistics.median(us[name])
    row = {"case": name, "label": args.label, "us_per_call_median": round(med, 2), "min": round(min(us[name]), 2), "max": round(max(us[name]), 2),
           "rounds": [round(x, 2) for x in us[name]], "calls_per_round": args.calls,
           "share_of_match": round(med * 1e-3 / statistics.median(match_ms), 4)}
    if name in votes:
        row.update({"atomic_candidates": votes[name], "target_pixels_covered": landed[name], "covered_share": round(landed[name] / N, 4),
                    "atomic_GB_per_s_over_the_call": round(8 * votes[name] / (med * 1e-6) / 1e9, 1), "float_add_yardstick_GB_per_s": 1300})
    print(json.dumps(row))
inst.close()
