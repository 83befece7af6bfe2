"""The device calls of the C host (csrc/sgm_host.c) are its behaviour: tests/host_trace_driver.c drives it through a list of scenarios on
the stand-in device (tests/stub_device.c), and

* the log of every step is compared with tests/golden/host_call_trace.json, recorded by tests/record_host_call_trace.py: the
  scenarios first_initialize .. default_instance from the host as it was before the buffers got one owner (reserve / k_buffers in
  sgm_host.c), the scenarios both_pageable .. result_in_four_pieces from the host as it was before the host-pointer entries got one
  result hand-over (queue_outputs / async_out in sgm_host.c), which printed the older scenarios as the first recording has them
  but for the one table drain init_path_difference accepts; the whole file again, with the scenarios right_view ..
  read_stages_wide_census and the roles of the post pass's buffers, from the host as it was before the cost-sum state, the post
  pass and the stage read-back got one owner each (sum_state / post_pass / k_stages in sgm_host.c);
* every allocation the scenarios perform is refused once, under AddressSanitizer + LeakSanitizer + UBSan."""
import json
import os
import re
import subprocess

import record_host_call_trace as REC
from standin import HOST_C

SYNC = ["sync", 0]


def collapse_syncs(log):
    out = []
    for e in log:
        if e == SYNC and out and out[-1] == SYNC:
            continue
        out.append(e)
    return out


def init_path_difference(want, got):
    """None when the two logs of an (re)initialize step agree: identical after collapsing each run of syncs into one, but for the
    drain upload_tables has in front of the allocation of tables that REPLACE existing ones (sync, alloc, alloc, h2d ...), which the
    recorded host lacked.  Otherwise a description of the first difference."""
    want, got = collapse_syncs(want), collapse_syncs(got)
    i = j = 0
    while i < len(want) or j < len(got):
        if i < len(want) and j < len(got) and want[i] == got[j]:
            i += 1
            j += 1
        elif j < len(got) and got[j] == SYNC and [e[0] for e in got[j + 1:j + 4]] == ["alloc", "alloc", "h2d"] and \
                (j == 0 or got[j - 1] != SYNC) and want[i:i + 3] == got[j + 1:j + 4]:
            j += 1
        else:
            return "entry %d: recorded %s, now %s" % (i, want[i:i + 3], got[j:j + 3])
    return None


def test_init_path_rule_accepts_only_the_tables_drain():
    a, h = ["alloc", 1], ["h2d", 64]
    assert init_path_difference([SYNC, SYNC, a], [SYNC, a]) is None
    assert init_path_difference([a, a, h, SYNC], [SYNC, a, a, h, SYNC]) is None
    assert init_path_difference([a, a, h], [a, SYNC, a, h]) is not None          # a drain anywhere else
    assert init_path_difference([SYNC, a, a, h], [a, a, h]) is not None          # a drain that went missing
    assert init_path_difference([a, h], [SYNC, a, h]) is not None
    assert init_path_difference([a, a, h], [a, a, h, h]) is not None


def test_device_calls_are_those_of_the_recorded_host(tmp_path):
    with open(REC.GOLDEN) as fh:
        want = json.load(fh)
    got = REC.record(HOST_C, str(tmp_path))
    assert list(got) == list(want), "the scenario list changed: record the golden trace again FROM THE PARENT COMMIT's sgm_host.c"
    drains = 0
    for name in want:
        assert [(s["path"], s["call"]) for s in got[name]] == [(s["path"], s["call"]) for s in want[name]], name
        for k, (w, g) in enumerate(zip(want[name], got[name])):
            if w["path"] == "frame":                 # the per-frame path: entry for entry
                assert g["log"] == w["log"], (name, k, w["call"])
            else:
                diff = init_path_difference(w["log"], g["log"])
                assert diff is None, (name, k, w["call"], diff)
                drains += len(collapse_syncs(g["log"])) - len(collapse_syncs(w["log"]))
    steps = sum(len(s) for s in want.values())
    calls = sum(len(st["log"]) for s in want.values() for st in s)
    print("%d scenarios, %d steps, %d recorded device calls; %d accepted table drains" % (len(want), steps, calls, drains))


# the allocation sites of sgm_host.c by the first message a refusal there prints (and the scenarios, where the message is the
# generic one of an abandoned match)
SITES = {
    "ensure_buffers": (r"device allocation failed for \d+x\d+x\d+$", None),
    "ensure_buffers (planes)": (r"path-cost planes", None),
    "ensure_S": (r"aggregated-cost volume", None),
    "ensure_cost": (r"for the cost volume", None),
    "ensure_fill": (r"hole-filling maps", None),
    "ensure_refine": (r"refinement maps", None),
    "sgm_initialize (extras)": (r"\(extras\)", None),
    "sgm_initialize (median scratch)": (r"\(median scratch\)", None),
    "prepare_costs (census64)": (r"the match was abandoned", ("census_7x7", "read_stages_wide_census")),
    "ensure_upsum": (r"the match was abandoned", ("fused_last_sweep", "fused_sweep_then_read_S", "fused_sweep_then_keep_stages")),
    "ensure_conf": (r"for the confidence map", None),
    "ensure_both": (r"maps of both views", None),
    "ensure_planes_io": (r"colour planes", None),
    "upload_census_need": (r"census block map", None),
    "upload_tables": (r"uploading path tables failed", None),
    "upload_rectify": (r"for the rectification of", None),
}


def test_every_allocation_refused_once_under_sanitizers(tmp_path):
    """Each allocation of each scenario is refused in a run of its own: the call that meets it returns false with the library's
    message, a reset at the same shape then succeeds, and destroying the instance leaves nothing behind."""
    exe = REC.build_driver(HOST_C, str(tmp_path), sanitize=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SGM_")}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    out = subprocess.run([exe, "refuse"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("host_trace_driver ok")
    reached = {}
    refusals = expected = 0
    block = []
    for line in out.stderr.splitlines():
        m = re.match(r"SCENARIO (\w+): (\d+) allocations", line)
        if m:
            expected += int(m.group(2)) - (1 if m.group(1) == "default_instance" else 0)    # but the one of its sgm_create
            block = []
        elif line.startswith("sgm_mi355x: "):
            block.append(line)
        elif line.startswith("REFUSED "):
            scenario = line.split()[1].rstrip(":")
            assert block, "no message from the library: " + line
            site = [s for s, (pat, where) in SITES.items() if re.search(pat, block[0]) and (where is None or scenario in where)]
            assert len(site) == 1, (line, block)
            reached[site[0]] = reached.get(site[0], 0) + 1
            refusals += 1
        elif line.startswith("RESET "):
            assert line.endswith(": ok"), line
            block = []
        else:
            raise AssertionError("unexpected output: " + line)
    assert refusals == expected and refusals > 0
    print("%d refused allocations; sites reached: %s" % (refusals, ", ".join("%s x%d" % kv for kv in sorted(reached.items()))))
    assert set(reached) == set(SITES), set(SITES) - set(reached)
