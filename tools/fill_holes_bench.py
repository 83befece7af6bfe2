"""Cost of the hole filling (sgm_set_fill_holes) on the bench's setup: KITTI-shaped frames (1242x375, D=128), batches of 8,
4 instances each driven by its own host thread through page-locked host pointers (sgm_reset + sgm_match_async +
sgm_match_wait), rounds alternating filling off / on.  Prints one JSON line per round, then the per-stage device time of one
instance alone (fill on: "lrcheck" includes the classification, "speckle" the three passes) and the worst case of the walks:
sgm_fill_holes on an all-INF batch (every pixel walks 8 x R steps in each of the three passes).

    python tools/fill_holes_bench.py [--rounds 4] [--seconds 3]
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
    ap.add_argument("--rounds", type=int, default=4)
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
        assert i.set_overlap_post(True)
        L, R, O = i.host_array((B, h, w), np.uint8), i.host_array((B, h, w), np.uint8), i.host_array((B, h, w), np.float32)
        for f in range(B):
            L[f], R[f] = S.synth_pair(w, h, d, 0x5EED0001 + k * B + f)
        insts.append(i)
        arrays.append((L, R, O))
    for fill in (False, True):                                    # warm-up of both settings
        for i in insts:
            assert i.set_fill_holes(fill)
        throughput(insts, arrays, w, h, opt, 1.0)
    for r in range(args.rounds * 2):
        fill = r % 2 == 1
        for i in insts:
            assert i.set_fill_holes(fill)
        fps = throughput(insts, arrays, w, h, opt, args.seconds)
        inv = float(np.isinf(arrays[0][2]).mean())
        print(json.dumps({"round": r, "fill_holes": fill, "fps": round(fps, 1), "invalid_share_last_map": round(inv, 4)}), flush=True)

    one = insts[0]
    L, R, O = arrays[0]
    for fill in (False, True):
        assert one.set_fill_holes(fill)
        assert one.reset(w, h, opt) and one.match(L, R) is not None        # warm-up
        one.enable_timing(True)
        for _ in range(20):
            assert one.reset(w, h, opt) and one.match_async(L, R, O) and one.match_wait()
        mean, mn, n = one.mean_timing()
        one.enable_timing(False)
        print(json.dumps({"alone": True, "fill_holes": fill, "matches": n, "mean_ms": {k: round(v, 4) for k, v in mean.items()},
                          "min_ms": {k: round(v, 4) for k, v in mn.items()}}), flush=True)

    assert one.reset(w, h, opt)
    t = torch.full((B, h, w), float("inf"), dtype=torch.float32, device="cuda")
    c = torch.full((B, h, w), 2, dtype=torch.uint8, device="cuda")
    ms = []
    for rep in range(6):
        t.fill_(float("inf"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert one.fill_holes(t.data_ptr(), c.data_ptr()) and one.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isinf(t).all())
    print(json.dumps({"worst_case": "all-INF batch, classes 2, three passes", "frames": B, "ms_host_timed": [round(x, 3) for x in ms[1:]]}))
    for i in insts:
        i.close()


if __name__ == "__main__":
    main()
