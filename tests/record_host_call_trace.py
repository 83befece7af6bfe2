"""Records the device-call trace of one csrc/sgm_host.c on the stand-in device (tests/host_trace_driver.c has the scenarios).

    python tests/record_host_call_trace.py PATH/TO/sgm_host.c [OUT.json]

The golden file tests/golden/host_call_trace.json is the trace of the host as it was BEFORE a change to sgm_host.c -- record it
from the parent commit's file (git show HEAD~:soc_project_stereo_matching_amd/csrc/sgm_host.c > /tmp/x/sgm_host.c), never from
the file under test: tests/test_host_call_trace.py replays the scenarios on the tree's file and compares."""
import json
import os
import subprocess
import sys
import tempfile

import standin

GOLDEN = os.path.join(standin.TESTS, "golden", "host_call_trace.json")


# launchers the driver wraps (-Wl,--wrap): it notes the roles of their pointers, then calls the stand-in's own
WRAPPED = ("alloc", "free", "speckle", "median", "lrcheck", "lrcheck_right", "d2d_async", "fill_classify", "fill_pass", "remap")


def build_driver(host_c, workdir, sanitize=False):
    """host_trace_driver + the given sgm_host.c + the stand-in device (and the stand-in remap) -> the executable (the headers are
    the tree's)"""
    wrap = "-Wl," + ",".join("--wrap=sgmd_" + n for n in WRAPPED)
    return standin.build(workdir, sanitize=sanitize, exe="host_trace_driver", host_c=host_c,
                         extra_sources=[os.path.join(standin.TESTS, "host_trace_driver.c"), os.path.join(standin.TESTS, "stub_rectify.c")],
                         flags=("-g", "-static-libasan", wrap) if sanitize else ("-g", wrap))


def record(host_c, workdir):
    exe = build_driver(host_c, workdir)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SGM_")}
    out = subprocess.run([exe, "trace"], capture_output=True, text=True, env=env, timeout=120)
    if out.returncode != 0:
        raise RuntimeError("host_trace_driver trace failed: " + out.stderr[-2000:])
    return json.loads(out.stdout)


def write(trace, path):
    """one step per line: a diff of two recordings reads step by step"""
    with open(path, "w") as fh:
        fh.write("{\n")
        for i, (name, steps) in enumerate(trace.items()):
            fh.write('  %s: [\n' % json.dumps(name))
            fh.write(",\n".join("    " + json.dumps(s) for s in steps))
            fh.write("\n  ]%s\n" % ("," if i + 1 < len(trace) else ""))
        fh.write("}\n")


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        trace = record(os.path.abspath(sys.argv[1]), tmp)
    dst = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    write(trace, dst)
    print("%s: %d scenarios, %d steps, %d device calls" % (dst, len(trace), sum(len(s) for s in trace.values()),
                                                          sum(len(st["log"]) for s in trace.values() for st in s)))
