"""Cost of the refinement (sgm_set_refine) on the bench's setup: KITTI-shaped frames (1242x375, D=128), batches of 8.

1. The refinement alone: sgm_refine_disparity on a batch of 8 maps (device time between two events on the instance's stream), at
   the default parameters and at T = 2 and 3.
2. Pipelined frame rate: 4 instances, each driven by its own host thread through page-locked host pointers (sgm_reset +
   sgm_match_async + sgm_match_wait), rounds alternating refinement off / on, with overlapped post passes off and on.
3. Per-stage device time of one instance alone, refinement off / on ("median" includes the refinement).

    python tools/refine_bench.py [--rounds 3] [--seconds 3]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def throughput(insts, arrays, w, h, opt, seconds):
    done = [0] * len(insts)
    stop = time.perf_counter() + seconds
    fail = []

    def worker(k):
        i, (L, R, O) = insts[k], arrays[k]
        while time.perf_counter() < stop:
            if not (i.reset(w, h, opt) and i.match_async(L, R, O) and i.match_wait()):
                fail.append(k)
                return
            done[k] += 1

    t0 = time.perf_counter()
    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(insts))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    el = time.perf_counter() - t0
    if fail:
        raise RuntimeError(f"a match failed on instances {sorted(set(fail))}")
    return sum(done) * insts[0].batch / el


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    import torch
    import soc_project_stereo_matching_amd as S
    w, h, d, B = 1242, 375, 128, args.batch
    opt = S.default_option(d)
    insts, arrays = [], []
    for k in range(args.instances):
        i = S.SGMInstance(0, batch=B)
        L, R, O = i.host_array((B, h, w), np.uint8), i.host_array((B, h, w), np.uint8), i.host_array((B, h, w), np.float32)
        for f in range(B):
            L[f], R[f] = S.synth_pair(w, h, d, 0x5EED0001 + k * B + f)
        insts.append(i)
        arrays.append((L, R, O))

    # 1. the refinement alone, on the maps and confidence of a real match
    one = insts[0]
    L, R, O = arrays[0]
    assert one.reset(w, h, opt)
    disp, conf = one.match_confidence(L, R)
    td0 = torch.from_numpy(disp).cuda()
    tc = torch.from_numpy(conf.view(np.int16)).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    st = torch.cuda.ExternalStream(one.stream)
    for params in ((S.REFINE_LAMBDA, S.REFINE_SIGMA, S.REFINE_ITERS), (S.REFINE_LAMBDA, S.REFINE_SIGMA, 2),
                   (S.REFINE_LAMBDA, S.REFINE_SIGMA, 3)):
        assert one.set_refine(True, *params)
        td = td0.clone()
        torch.cuda.synchronize()
        ms = []
        for rep in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                td.copy_(td0)
                e0.record(st)
            assert one.refine_disparity(td, tc, tg)
            with torch.cuda.stream(st):
                e1.record(st)
            assert one.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = sorted(ms[2:])
        print(json.dumps({"alone": "sgm_refine_disparity", "frames": B, "params": params, "launches": 2 * params[2],
                          "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}), flush=True)
    assert one.set_refine(False)

    # 2. pipelined frame rate
    for overlap in (False, True):
        for i in insts:
            assert i.set_overlap_post(overlap)
        for refine in (False, True):                              # warm-up of both settings
            for i in insts:
                assert i.set_refine(refine)
            throughput(insts, arrays, w, h, opt, 1.0)
        for r in range(args.rounds * 2):
            refine = r % 2 == 1
            for i in insts:
                assert i.set_refine(refine)
            fps = throughput(insts, arrays, w, h, opt, args.seconds)
            inv = float(np.isinf(arrays[0][2]).mean())
            print(json.dumps({"overlap_post": overlap, "round": r, "refine": refine, "fps": round(fps, 1),
                              "invalid_share_last_map": round(inv, 4)}), flush=True)

    # 3. per-stage device time of one instance alone
    assert one.set_overlap_post(False)
    for refine in (False, True):
        assert one.set_refine(refine)
        assert one.reset(w, h, opt) and one.match(L, R) is not None        # warm-up
        one.enable_timing(True)
        for _ in range(20):
            assert one.reset(w, h, opt) and one.match_async(L, R, O) and one.match_wait()
        mean, mn, n = one.mean_timing()
        one.enable_timing(False)
        print(json.dumps({"stages": True, "refine": refine, "matches": n, "mean_ms": {k: round(v, 4) for k, v in mean.items()},
                          "min_ms": {k: round(v, 4) for k, v in mn.items()}}), flush=True)
    for i in insts:
        i.close()


if __name__ == "__main__":
    main()
