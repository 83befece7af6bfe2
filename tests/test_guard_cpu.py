"""The debug allocation mode's bookkeeping (csrc/sgm_guard.h) without a GPU: tests/guard_driver.c includes the header with malloc
as the device and runs under ASan + UBSan as a program of its own.  Pad arithmetic, two allocations of one size, a byte planted at
either end of either band (side and offset of the report), the poison-valued byte nobody can see (why the GPU tests run under two
poisons), the sticky count of a violated buffer that was freed, unregistered pointers, four threads.  tests/test_gpu_guard_bands.py
is the mode at work on the device."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_guard_registry_is_right_and_asan_ubsan_clean(tmp_path):
    exe = os.path.join(str(tmp_path), "guard_driver")
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "guard_driver.c"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("guard_driver ok")


def test_the_mode_is_off_without_a_device():
    """The exported check with nothing under guard: 0 violations, 0 live allocations, 0 bytes (needs no GPU: nothing to copy)."""
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
