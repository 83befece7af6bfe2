#!/usr/bin/env bash
# refresh_profiles.sh OUTDIR [STEP...] -- run on an MI355X: collects everything profiles/ holds for the current kernels into OUTDIR;
# copy the files into profiles/ afterwards with `python tools/adopt_profiles.py NN OUTDIR`.
# Steps (default: all, in this order): counters:WORKLOAD for the four counter workloads, stats, bench.  Every step runs under a time
# limit of its own and the first one that fails ends the run: nothing more is started on a GPU that has just faulted or hung.
# Where one call cannot take them all, run them in several, with the same OUTDIR (counters.json collects the workloads; `stats` and
# `bench` read profiles/counters.json, which `stats` takes from OUTDIR).
set -euxo pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)}
OUT=$(mkdir -p "${1:?usage: refresh_profiles.sh OUTDIR [STEP...]}" && cd "$1" && pwd)
shift
WLS="kitti_1242x375_d128_p8 cone_450x375_d64_p8 drivingstereo_1762x800_d192_p8 middlebury_2880x1988_d256_p8"
[ $# -gt 0 ] || set -- $(for wl in $WLS; do echo counters:$wl; done) stats bench
export TMPDIR=/tmp
for step in "$@"; do
  case $step in
  counters:*)       # five rocprofv3 --pmc passes, each in a run of its own (tools/profile_counters.py)
    wl=${step#counters:}
    (cd /tmp && timeout -k 10 420 python3 $R/tools/profile_counters.py --workload $wl --out $OUT/counters.json --scratch $OUT/counters > $OUT/counters_$wl.log 2>&1) \
      || { tail -5 $OUT/counters_$wl.log; exit 1; }
    tail -2 $OUT/counters_$wl.log ;;
  stats)
    cp $OUT/counters.json $R/profiles/counters.json          # so that the bench runs below read fresh counters
    # the headline loop under the kernel trace: per-kernel calls / average duration of the timed configuration.  60 timed steps after 2
    # warm-up steps (248 launches per kernel, 8 of them warm-up) so that the CSV's average over ALL calls and the JSON line's average
    # over the timed launches describe nearly the same set; tools/trace_summary.py gives the timed-only mean from the trace.
    rm -rf $OUT/prof_stats
    (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -o stats --output-format csv -- python3 $R/bench.py --gpus 1 --steps 60 --warmup 2 > $OUT/bench_under_rocprof.json 2> $OUT/prof_stats.log) \
      || { tail -5 $OUT/prof_stats.log; exit 1; }
    python3 $R/tools/trace_summary.py $OUT/prof_stats/stats_kernel_trace.csv $OUT/bench_under_rocprof.json > $OUT/kernel_trace_summary.json ;;
  bench)
    (cd $R && timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err) || { tail -5 $OUT/bench.err; exit 1; }
    cp $R/bench_detail.json $OUT/ ;;
  *) echo "unknown step $step"; exit 2 ;;
  esac
done
