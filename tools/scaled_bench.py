"""What matching at 1/f scale costs and saves (NOTES.md section 25) -- needs an MI355X.

    python tools/scaled_bench.py [--cases 4k,middlebury,kitti8] [--rounds 7] [--calls 12] [--warmup 3] [--full-only]

Device-resident SGM_SynthPair frames.  Per case the full-resolution match (sgm_reset + sgm_match_device) and, per factor, the
composed call (sgm_reset + sgm_match_scaled_device on an instance of the low-resolution shape with D / f disparities): `warmup`
calls, then `calls` calls queued back to back and one synchronise; time per call = wall clock / calls; median, minimum and maximum
over `rounds`.  The parts of the composed call are timed on their own with HIP events on the instance's stream, queued back to
back the same way: the small match alone, the two downscale launches, the re-search kernel (sgm_upscale_disparity on the real
small map and the real full-resolution census words, read back from the full-resolution instance) and the guided selection alone
(radius -1).  The full-resolution census is the "census" entry of the full-resolution instance's own stage timing (the same
launcher on the same geometry).  Bytes the downscale must move: the f x f blocks read + the samples written, both views.  Popcount
terms of the re-search: pixels x (2r+1)^2 x (2f+1).  --full-only stops after the full-resolution matches (SGM_LIBRARY_PATH may
point the run at the library of another commit).  One JSON line per measurement."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import soc_project_stereo_matching_amd as S

CASES = {   # W, H, full-resolution D, batch, factors
    "4k": (3840, 2160, 256, 1, (2, 4)),
    "middlebury": (2880, 1988, 256, 1, (2,)),
    "kitti8": (1242, 375, 128, 8, (2,)),
}
ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="4k,middlebury,kitti8")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--full-only", action="store_true")
args = ap.parse_args()
RADIUS, PENALTY = S.sgm.SCALE_DEFAULT_RADIUS, S.sgm.SCALE_DEFAULT_PENALTY


def summary(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def wall_ms(inst, call):
    """ms per call: calls queued back to back, one synchronise"""
    for _ in range(args.warmup):
        call()
    assert inst.synchronize()
    out = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        assert inst.synchronize()
        out.append((time.perf_counter() - t0) / args.calls * 1e3)
    return out


def event_us(inst, call):
    """us per call between two events on the instance's stream"""
    stream = torch.cuda.ExternalStream(inst.stream)
    for _ in range(args.warmup):
        call()
    out = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            call()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / args.calls * 1e3)
    return out


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


for name in args.cases.split(","):
    W, H, D, B, factors = CASES[name]
    pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
    left, right = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    opt = S.default_option(D)
    full = S.SGMInstance(0, batch=B)

    def match_full():
        assert full.reset(W, H, opt) and full.match_device(left.data_ptr(), right.data_ptr(), disp.data_ptr())

    if not full.reset(W, H, opt):                                 # beyond what the library admits at full resolution
        print(json.dumps({"case": name, "what": "full-resolution match", "shape": [B, H, W], "D": D, "refused": True}), flush=True)
        full.close()
        continue
    ms_full = wall_ms(full, match_full)
    full.enable_timing(True)
    for _ in range(args.calls):
        match_full()
    assert full.synchronize()
    stage_mean, _, n_timed = full.mean_timing()
    full.enable_timing(False)
    census_us = stage_mean["census"] * 1e3
    print(json.dumps({"case": name, "what": "full-resolution match", "shape": [B, H, W], "D": D, "ms_per_call": summary(ms_full),
                      "frames_per_s": round(B / statistics.median(ms_full) * 1e3, 1), "library": os.path.relpath(S.library_path(), ROOT),
                      "finite_share": round(float(torch.isfinite(disp).float().mean()), 4)}), flush=True)
    if args.full_only:
        full.close()
        continue
    words = [dev(np.stack([(full.select_frame(k), full.read_stage(v))[1] for k in range(B)])) for v in (0, 1)]
    full.close()
    for f in factors:
        w, h, Ds = W // f, H // f, D // f
        small_opt = S.default_option(Ds)
        inst = S.SGMInstance(0, batch=B)
        assert inst.initialize(w, h, small_opt)
        spec = S.scale_spec(W, H, f, frames=B, radius=RADIUS, penalty=PENALTY, d_lo=0, d_hi=f * Ds - 1)
        out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")

        def match_scaled():
            assert inst.reset(w, h, small_opt) and inst.match_scaled_device(spec, left.data_ptr(), right.data_ptr(), out.data_ptr())

        ms_scaled = wall_ms(inst, match_scaled)
        # the parts, on buffers of the tool's own
        sl = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
        sr = torch.empty_like(sl)
        small = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        assert inst.downscale(spec, left.data_ptr(), sl.data_ptr()) and inst.downscale(spec, right.data_ptr(), sr.data_ptr())

        def match_small():
            assert inst.reset(w, h, small_opt) and inst.match_device(sl.data_ptr(), sr.data_ptr(), small.data_ptr())

        ms_small = wall_ms(inst, match_small)
        up = torch.empty_like(out)
        us_down = event_us(inst, lambda: inst.downscale(spec, left.data_ptr(), sl.data_ptr()) and inst.downscale(spec, right.data_ptr(), sr.data_ptr()))
        us_up = event_us(inst, lambda: inst.upscale_disparity(spec, small.data_ptr(), sl.data_ptr(), left.data_ptr(), words[0].data_ptr(),
                                                              words[1].data_ptr(), False, up.data_ptr()))
        prior_spec = S.scale_spec(W, H, f, frames=B, radius=-1)
        us_prior = event_us(inst, lambda: inst.upscale_disparity(prior_spec, small.data_ptr(), sl.data_ptr(), left.data_ptr(), None, None,
                                                                 False, out.data_ptr()))
        match_scaled()
        assert inst.synchronize()
        same = bool(torch.equal(out.view(torch.int32), up.view(torch.int32)))      # the parts are the composed call's
        px = B * W * H
        down_bytes = 2 * (B * (w * f) * (h * f) + B * w * h)
        terms = px * (2 * RADIUS + 1) ** 2 * (2 * f + 1)
        med = statistics.median
        added = (med(us_down) + census_us + med(us_up)) * 1e-3
        print(json.dumps({"case": name, "what": f"scaled match f={f}", "small_shape": [B, h, w], "small_D": Ds,
                          "ms_per_call": summary(ms_scaled), "frames_per_s": round(B / med(ms_scaled) * 1e3, 1),
                          "speedup_over_full": round(med(ms_full) / med(ms_scaled), 2),
                          "small_match_ms": summary(ms_small), "small_match_share_of_full": round(med(ms_small) / med(ms_full), 4),
                          "one_over_f_cubed": round(1 / f ** 3, 4),
                          "downscale_both_views_us": summary(us_down, 2), "downscale_bytes": down_bytes,
                          "downscale_GB_per_s": round(down_bytes / (med(us_down) * 1e-6) / 1e9, 1),
                          "census_full_resolution_us": round(census_us, 2),
                          "research_us": summary(us_up, 2), "research_popcount_terms": terms,
                          "research_Gterms_per_s": round(terms / (med(us_up) * 1e-6) / 1e9, 1),
                          "guided_selection_alone_us": summary(us_prior, 2),
                          "added_full_resolution_ms": round(added, 4), "added_share_of_scaled_call": round(added / med(ms_scaled), 4),
                          "parts_equal_composed": same,
                          "finite_share": round(float(torch.isfinite(up).float().mean()), 4)}), flush=True)
        inst.close()
