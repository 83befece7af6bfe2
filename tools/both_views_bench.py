"""Device time of both views' maps from one match against two single-view matches (NOTES.md section 15) -- needs an MI355X.

    [SGM_LIBRARY_PATH=other/libsgm_mi355x.so] python tools/both_views_bench.py both|two|plain LABEL

KITTI 1242x375, D = 128, 8 paths, batch 8, device-resident frames.  One call = sgm_reset + sgm_match_both_device (both), or
sgm_reset + sgm_match_device with reference view 0 and again with view 1 (two), or one plain sgm_reset + sgm_match_device (plain).
20 warm-up calls, then 9 rounds of 40 calls queued back to back and one synchronize each: wall clock / 40 per round.  Prints one
JSON line with every round, their median, minimum and maximum.  SGM_LIBRARY_PATH points an A/B run at a build of other sources (a
library without sgm_match_both can run `two` and `plain`)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import soc_project_stereo_matching_amd as S
mode, label = sys.argv[1], sys.argv[2]
W, H, D, B = 1242, 375, 128, 8
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
o0 = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
o1 = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
inst = S.SGMInstance(0, batch=B)
def step():
    if mode == "both":
        assert inst.reset(W, H, opt) and inst.match_both_device(l.data_ptr(), r.data_ptr(), o0.data_ptr(), o1.data_ptr())
    elif mode == "two":
        inst.set_reference_view(False)
        assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), o0.data_ptr())
        inst.set_reference_view(True)
        assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), o1.data_ptr())
    else:
        assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), o0.data_ptr())
for _ in range(20):
    step()
assert inst.synchronize()
rounds = []
N = 40
for _ in range(9):
    t0 = time.perf_counter()
    for _ in range(N):
        step()
    assert inst.synchronize()
    rounds.append((time.perf_counter() - t0) / N * 1e3)
print(json.dumps({"label": label, "mode": mode, "ms_per_batch_median": round(statistics.median(rounds), 4), "min": round(min(rounds), 4),
                  "max": round(max(rounds), 4), "rounds": [round(x, 4) for x in rounds], "iterations_per_round": N,
                  "valid_left": int(torch.isfinite(o0).sum()), "valid_right": int(torch.isfinite(o1).sum()) if mode != "plain" else None}))
inst.close()
