"""The product's C host (csrc/sgm_host.c, and the multi-GPU host csrc/sgm_tiles.c + sgm_tile_sched.c with ranks as threads) is AddressSanitizer / UBSan clean when driven through every entry-point family
with the stub device layer (tests/stub_device.c) -- no GPU; sanitizers are only available for the CPU build."""
import os
import shutil
import subprocess

import pytest

import standin


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_is_asan_ubsan_clean(tmp_path):
    exe = standin.build(tmp_path, sanitize=True, exe="host_sanitize_driver", extra_sources=standin.SANITIZE_DRIVER)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("host_sanitize_driver ok")
