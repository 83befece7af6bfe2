"""What 16-bit input costs a call and what it buys (NOTES.md section 23) -- needs an MI355X.

    python tools/pixels16_bench.py [--rounds 7] [--calls 40] [--eight-only]

KITTI 1242x375, D = 128, 8 paths, batch 8, device-resident frames.  One call = sgm_reset + sgm_match_device.  Instances in one
process, visited by turns:
    c8a, c8b   8-bit input, the reference's 5x5 centre census, twice: what separates them is the noise floor of the method
    c12        12-bit input (the same frames << 4: the results must be, and are checked to be, those of c8a), 5x5 centre census
    s8, s12    the symmetric 7x7 census on 8- and on 12-bit input
20 warm-up calls each, then `rounds` rounds of `calls` calls queued back to back and one synchronize, wall clock / calls.  Then, in
passes of their own: the mean device time per stage over 20 calls per case with sgm_enable_timing ("census", and the sum of the
eight stages = the match), and the remap alone in both depths -- sgm_rectify queued 200 times back to back, wall clock / calls.
The bytes the census moves per batch: reads 2 views x B x W x H samples (1 or 2 bytes), writes 2 x B x W x H words of 4 bytes and,
with more than 8 bits, 2 x B x W x H narrowed bytes.
--eight-only: the 8-bit cases alone, for a build without the feature (SGM_LIBRARY_PATH names the library): the parent's numbers in
the same session.
What it buys: the cone pair as a 4-stop-underexposed 12-bit frame (v = u8, bits = 12), matched through the 12-bit path and, after
narrowing (v >> 4), through the 8-bit one; bad pixels (+INF or more than 1 px off) over the pixels with known ground truth
(tests/golden/gt_disparity.npz), as NOTES.md section 18 scored the symmetric census.  Prints one JSON line per case."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import soc_project_stereo_matching_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--eight-only", action="store_true")
args = ap.parse_args()
W, H, D, B = 1242, 375, 128, 8
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l8, r8 = (np.stack([p[v] for p in pairs]) for v in (0, 1))
dev = {8: (torch.from_numpy(l8).cuda(), torch.from_numpy(r8).cuda())}
if not args.eight_only:
    # uint16 frames as bytes: torch need not know the type
    dev[12] = tuple(torch.from_numpy((a.astype(np.uint16) << 4).view(np.uint8)).cuda() for a in (l8, r8))
out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)


def library_label():
    """the library measured, as it goes into profiles/: the in-tree one by its path in the repository, a build named by
    SGM_LIBRARY_PATH by a label -- never an absolute path of the machine that measured"""
    path = os.path.realpath(S.library_path())
    root = os.path.realpath(ROOT) + os.sep
    if not os.environ.get("SGM_LIBRARY_PATH") and path.startswith(root):
        return path[len(root):]
    return "<parent build>/" + os.path.basename(path)


cases = {"c8a": (8, 0), "c12": (12, 0), "s8": (8, 1), "s12": (12, 1), "c8b": (8, 0)}
if args.eight_only:
    cases = {k: v for k, v in cases.items() if v[0] == 8}
inst = {}
for name, (bits, sym) in cases.items():
    i = S.SGMInstance(0, batch=B)
    if sym:
        assert i.set_census_kind(S.sgm.CENSUS_SYMMETRIC) and i.set_census_window(7, 7)
    if bits > 8:
        assert i.set_pixel_bits(bits)
    inst[name] = i


def step(name):
    i = inst[name]
    l, r = dev[cases[name][0]]
    assert i.reset(W, H, opt) and i.match_device(l.data_ptr(), r.data_ptr(), out.data_ptr())


maps = {}
for name in inst:
    for _ in range(20):
        step(name)
    assert inst[name].synchronize()
    maps[name] = out.cpu().numpy().copy()
if not args.eight_only:
    for a, b in (("c12", "c8a"), ("s12", "s8")):
        assert np.array_equal(maps[a].view(np.uint32), maps[b].view(np.uint32)), f"{a} differs from {b}"
rounds = {name: [] for name in inst}
for _ in range(args.rounds):
    for name in inst:
        t0 = time.perf_counter()
        for _ in range(args.calls):
            step(name)
        assert inst[name].synchronize()
        rounds[name].append((time.perf_counter() - t0) / args.calls * 1e3)
stages = {}
for name, i in inst.items():
    i.enable_timing(True)
    for _ in range(20):
        step(name)
    assert i.synchronize()
    mean, _, n = i.mean_timing()
    assert n == 20
    stages[name] = mean
    i.enable_timing(False)
med = {name: statistics.median(v) for name, v in rounds.items()}
for name, (bits, sym) in cases.items():
    moved = 2 * B * W * H * ((2 if bits > 8 else 1) + 4 + (1 if bits > 8 else 0))
    print(json.dumps({"case": name, "bits": bits, "census": "symmetric 7x7" if sym else "centre 5x5", "library": library_label(),
                      "ms_per_batch_median": round(med[name], 4), "min": round(min(rounds[name]), 4), "max": round(max(rounds[name]), 4),
                      "rounds": [round(x, 4) for x in rounds[name]], "calls_per_round": args.calls,
                      "census_mean_ms": round(stages[name]["census"], 4), "match_mean_ms": round(sum(stages[name].values()), 4),
                      "census_bytes": moved, "census_GB_per_s": round(moved / (stages[name]["census"] * 1e-3) / 1e9, 1),
                      "valid_pixels": int(np.isfinite(maps[name]).sum())}))
summary = {"noise_floor_ms": round(abs(med["c8a"] - med["c8b"]), 4), "c8_ms": round((med["c8a"] + med["c8b"]) / 2, 4)}
if not args.eight_only:
    import rectify_ref as RR
    summary.update({"c12_minus_c8_ms": round(med["c12"] - summary["c8_ms"], 4), "s12_minus_s8_ms": round(med["s12"] - med["s8"], 4),
                    "census_c12_minus_c8_ms": round(stages["c12"]["census"] - (stages["c8a"]["census"] + stages["c8b"]["census"]) / 2, 4),
                    "census_s12_minus_s8_ms": round(stages["s12"]["census"] - stages["s8"]["census"], 4)})
    m = (*RR.model_maps(RR.SMALL, W, H), *RR.model_maps(RR.SMALL, W, H, sign=-1.0))
    for name, bits in (("c8a", 8), ("c12", 12)):
        i = inst[name]
        assert i.set_rectify(*m) and i.reset(W, H, opt)
        l, r = dev[bits]
        rl, rr = torch.empty_like(l), torch.empty_like(r)
        torch.cuda.synchronize()
        alone = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(200):
                assert i.rectify(l.data_ptr(), r.data_ptr(), rl.data_ptr(), rr.data_ptr())
            assert i.synchronize()
            alone.append((time.perf_counter() - t0) / 200 * 1e3)
        moved = 2 * 8 * W * H + 2 * B * 2 * W * H * (2 if bits > 8 else 1)
        k_ms = statistics.median(alone)
        summary[f"remap_{bits}_bits"] = {"alone_ms": round(k_ms, 4), "min_ms": round(min(alone), 4), "bytes": moved,
                                         "GB_per_s": round(moved / (k_ms * 1e-3) / 1e9, 1)}
print(json.dumps(summary))
for i in inst.values():
    i.close()

if not args.eight_only:
    # what it buys: the cone pair as a 12-bit frame that uses its lowest 8 bits only
    from conftest import load_npz, option_from_dict
    with open(os.path.join(ROOT, "tests", "golden", "cases.json")) as f:
        case = {c["name"]: c for c in json.load(f)["cases"]}["cone"]
    z = load_npz("cone_inputs.npz")
    left, right = z["left"], z["right"]
    copt = option_from_dict(case["option"])
    gt = load_npz("gt_disparity.npz")
    truth, known = gt["cone"].astype(np.float32) / gt["cone_scale"], gt["cone"] > 0
    h, w = left.shape
    rate = {}
    for name, bits, imgs in (("12-bit path", 12, (left.astype(np.uint16), right.astype(np.uint16))),
                             ("narrowed to 8 bits (v >> 4)", 8, (left >> 4, right >> 4)), ("the 8-bit original", 8, (left, right))):
        i = S.SGMInstance(0)
        assert i.set_pixel_bits(bits) and i.reset(w, h, copt)
        d = i.match(*imgs)
        i.close()
        bad = ~np.isfinite(d) | (np.abs(d - truth) > 1)
        rate[name] = round(100 * float(bad[known].mean()), 2)
    print(json.dumps({"cone_bad_pixels_percent": rate}))
