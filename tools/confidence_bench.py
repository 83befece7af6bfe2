"""Cost of the matching confidence (sgm_match_confidence*) on the bench's setup: KITTI-shaped frames (1242x375, D=128), batches
of 8, 4 instances each driven by its own host thread through page-locked host pointers (sgm_reset + sgm_match_async /
sgm_match_confidence_async + sgm_match_wait; with confidence the uint16 map comes back as well), rounds alternating confidence
off / on.  Prints one JSON line per round, then the per-stage device time of one instance alone with and without it (the store
counts toward "sum", the cost-sum + WTA kernel).

    python tools/confidence_bench.py [--rounds 4] [--seconds 3]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def throughput(insts, arrays, w, h, opt, seconds, conf):
    done = [0] * len(insts)
    stop = time.perf_counter() + seconds
    fail = []

    def worker(k):
        i, (L, R, O, Cf) = insts[k], arrays[k]
        while time.perf_counter() < stop:
            if not (i.reset(w, h, opt) and (i.match_confidence_async(L, R, O, Cf) if conf else i.match_async(L, R, O))
                    and i.match_wait()):
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
    import soc_project_stereo_matching_amd as S
    w, h, d, B = 1242, 375, 128, args.batch
    opt = S.default_option(d)
    insts, arrays = [], []
    for k in range(args.instances):
        i = S.SGMInstance(0, batch=B)
        assert i.set_overlap_post(True)
        L, R = i.host_array((B, h, w), np.uint8), i.host_array((B, h, w), np.uint8)
        O, Cf = i.host_array((B, h, w), np.float32), i.host_array((B, h, w), np.uint16)
        for f in range(B):
            L[f], R[f] = S.synth_pair(w, h, d, 0x5EED0001 + k * B + f)
        insts.append(i)
        arrays.append((L, R, O, Cf))
    for conf in (False, True):                                    # warm-up of both settings
        throughput(insts, arrays, w, h, opt, 1.0, conf)
    fps = {False: [], True: []}
    for r in range(args.rounds * 2):
        conf = r % 2 == 1
        f = throughput(insts, arrays, w, h, opt, args.seconds, conf)
        fps[conf].append(f)
        print(json.dumps({"round": r, "confidence": conf, "fps": round(f, 1)}), flush=True)
    med = {k: float(np.median(v)) for k, v in fps.items()}
    print(json.dumps({"pipelined_fps_median": {"plain": round(med[False], 1), "confidence": round(med[True], 1)},
                      "ratio": round(med[True] / med[False], 4)}), flush=True)

    one = insts[0]
    L, R, O, Cf = arrays[0]
    for conf in (False, True):
        assert one.reset(w, h, opt) and (one.match_confidence(L, R) if conf else one.match(L, R)) is not None   # warm-up
        one.enable_timing(True)
        for _ in range(20):
            assert one.reset(w, h, opt)
            assert (one.match_confidence_async(L, R, O, Cf) if conf else one.match_async(L, R, O)) and one.match_wait()
        mean, mn, n = one.mean_timing()
        one.enable_timing(False)
        print(json.dumps({"alone": True, "confidence": conf, "matches": n, "mean_ms": {k: round(v, 4) for k, v in mean.items()},
                          "min_ms": {k: round(v, 4) for k, v in mn.items()}}), flush=True)
    for i in insts:
        i.close()


if __name__ == "__main__":
    main()
