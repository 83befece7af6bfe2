"""The C stream driver with the temporal filter on (csrc/sgm_stream.c --temporal): one instance is one stream, the frames of its
batches are consecutive frames (sequence = 1), and the per-frame sgm_reset keeps the history.  Its hash of the last frame of batch 0
must be the oracle's maps of frames 0 .. B - 1 pushed through tests/temporal_ref.py in order; frame 0 meets an empty history, so
its hash stays the oracle's own."""
import json
import os
import subprocess

import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_stream")


def fnv1a(b: bytes) -> str:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_c_stream_driver_filters_across_the_frames_of_a_batch(oracle):
    from oracle.pyoracle import default_option
    assert os.path.exists(EXE), "sgm_stream is not built"
    w, h, d, seed, batch = 320, 96, 64, 77, 4
    opt = default_option(d)
    finals = [oracle.run(*oracle.synth_pair(w, h, d, seed + i), opt)["final"] for i in range(batch)]
    rows = TC.filtered(TR.Spec(0.4, 0.125, 3, 2), finals)
    out = subprocess.run([EXE, "--temporal", "0.4,0.125,3,2", "--instances", "1", "--batch", str(batch), "--frames", "8", "--width", str(w),
                          "--height", str(h), "--disparities", str(d), "--seed", str(seed), "--seconds", "0.5"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-800:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["hash_temporal"] == fnv1a(np.ascontiguousarray(rows[batch - 1][0]).tobytes())
    assert line["hash_frame0"] == fnv1a(np.ascontiguousarray(finals[0]).tobytes())
    assert rows[batch - 1][3][1] > 1000 and not np.array_equal(rows[batch - 1][0], finals[batch - 1])     # the filter did something
    assert line["frames"] >= 2 * batch and not line.get("failed", False)
