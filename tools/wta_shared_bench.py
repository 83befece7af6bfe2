"""Device time of the cost-sum / winner-take-all stages for an A/B run of two builds (NOTES.md section 22) -- needs an MI355X.

    [SGM_LIBRARY_PATH=other/libsgm_mi355x.so] [SGM_FUSED_WTA=0 | SGM_UPSUM=1] python tools/wta_shared_bench.py kitti|d512 LABEL

kitti: 1242x375, D = 128, 8 paths, batch 8 (SGM_FUSED_WTA=0: sgm_sum_wta_k + sgm_wta_right_k instead of the row kernel;
SGM_UPSUM=1: the fused last sweep).  d512: 1242x375, D = 512, batch 2 (always the separate kernels: the row kernel stops at
Dp = 256).  Device-resident frames, one instance alone on the GPU; 10 warm-up matches, then 5 rounds of 30 matches with the
library's per-stage HIP events (sgm_mean_timing).  Prints one JSON line: per round the mean `sum` and `wta` stage times, their
medians, and the digest of the last map (two builds must agree on it)."""
import hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import soc_project_stereo_matching_amd as S
shape, label = sys.argv[1], sys.argv[2]
W, H, D, B = {"kitti": (1242, 375, 128, 8), "d512": (1242, 375, 512, 2)}[shape]
pairs = [S.synth_pair(W, H, D, 0x5EED0002 + k) for k in range(B)]
l = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
r = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
opt = S.default_option(D)
inst = S.SGMInstance(0, batch=B)
def step():
    assert inst.reset(W, H, opt) and inst.match_device(l.data_ptr(), r.data_ptr(), out.data_ptr())
for _ in range(10):
    step()
assert inst.synchronize()
rounds = []
for _ in range(5):
    inst.enable_timing(True)
    for _ in range(30):
        step()
        assert inst.synchronize()
    mean, _, n = inst.mean_timing()
    inst.enable_timing(False)
    assert n == 30
    rounds.append({k: round(mean[k], 4) for k in ("sum", "wta")})
print(json.dumps({"label": label, "shape": shape, "env": {k: os.environ[k] for k in ("SGM_FUSED_WTA", "SGM_UPSUM") if k in os.environ},
                  "fused_sweep_rows": inst.fused_sweep_rows(),
                  "sum_ms_median": statistics.median(x["sum"] for x in rounds), "wta_ms_median": statistics.median(x["wta"] for x in rounds),
                  "rounds": rounds, "sha256_out": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}))
inst.close()
