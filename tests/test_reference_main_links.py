"""The REFERENCE's own driver (SemiGlobalMatching/main.c:72,83) linked against libsgm_mi355x.so instead of the reference's
SemiGlobalMatching.c, exactly the command INTEGRATION.md section 2 gives a maintainer: oracle/build_ref.sh main compiles it in place
(nothing is copied into the repo) into oracle/_ref/sgm_ref_main when build() runs where the reference is present.  Proves the
drop-in claim at link level: the three entry points and the SGMOption layout the reference's caller was compiled against resolve
to this library.  Its inputs and the PNG the reference committed are data fixtures under tests/golden/ (cone_im2.png, cone_im6.png,
cone_im2.d.png).

Skips where oracle/_ref/sgm_ref_main was not built (no reference where build() ran)."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "oracle", "_ref", "sgm_ref_main")

pytestmark = pytest.mark.skipif(not os.path.isfile(EXE), reason="oracle/_ref/sgm_ref_main not built (needs the reference)")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    d = tmp_path_factory.mktemp("refmain")
    (d / "bin").mkdir()
    # the driver's paths are relative ("../Data/cone/..."): run it from a private bin/ beside a Data/cone with links to the two
    # inputs, so that its output PNG is written next to them in the temporary directory
    cone = d / "Data" / "cone"
    cone.mkdir(parents=True)
    for f in ("im2.png", "im6.png"):
        os.symlink(os.path.join(GOLDEN, f"cone_{f}"), cone / f)
    return d / "bin"


def test_reference_main_links_against_the_library(exe):
    und = subprocess.check_output(["nm", "-D", "--undefined-only", EXE], text=True)
    for sym in ("SGM_Initialize", "SGM_Match"):
        assert sym in und                                           # resolved at run time ...
    ldd = subprocess.check_output(["ldd", EXE], text=True)
    assert "libsgm_mi355x.so" in ldd and "not found" not in ldd     # ... by this library
    assert "sgm" not in [l.split()[-1] for l in und.splitlines()]  # the reference's global instance is not needed


def test_reference_main_runs_to_the_library(exe):
    """Without a GPU the run must end where the library says 'no device' (exit code -2 = main.c:74-78), with a GPU it
    must write the PNG the reference committed (all but the one undefined-behaviour pixel)."""
    import torch
    p = subprocess.run([EXE], cwd=str(exe), capture_output=True, text=True, timeout=120)
    if not torch.cuda.is_available():
        assert p.returncode == 254 and "SGM initialization failed" in p.stdout
        assert "no HIP device" in p.stderr
        return
    assert p.returncode == 0, p.stdout + p.stderr
    import numpy as np
    from PIL import Image
    got = np.asarray(Image.open(exe.parent / "Data" / "cone" / "im2.d.png"))
    want = np.asarray(Image.open(os.path.join(GOLDEN, "cone_im2.d.png")))
    assert np.argwhere(got != want).tolist() == [[374, 153]]
