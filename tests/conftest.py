import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    import shutil
    lib = os.path.join(ROOT, "soc_project_stereo_matching_amd", "libsgm_mi355x.so")
    if not os.path.exists(lib) and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        # a fresh checkout: the library is git-ignored; cross-compile it (no GPU needed, ~40 s) so that the C-ABI
        # tests have something to load.  The product itself never builds or falls back at run time.
        import subprocess
        subprocess.call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")],
                        stdout=subprocess.DEVNULL)


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def golden_cases():
    cases = {}
    # cases.json: make_golden.py; cases_scenes.json: make_golden_scenes.py (the reference's Cloth3 / Reindeer / Wood2 pairs)
    # cases_paths4.json: make_golden_paths4.py (the 4-path mode = the reference's first four CostAggregate calls)
    for name in ("cases.json", "cases_scenes.json", "cases_paths4.json"):
        with open(os.path.join(GOLDEN, name)) as f:
            cases.update({c["name"]: c for c in json.load(f)["cases"]})
    return cases


def option_from_dict(d):
    from oracle.pyoracle import SGMOption
    o = SGMOption()
    for k, v in d.items():
        setattr(o, k, v)
    return o


def load_npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case_inputs(case, oracle):
    """Inputs of a golden case: stored arrays for tiny cases / cone, else regenerated from the seed
    with the LCG generator and verified against the stored input digests."""
    from oracle.pyoracle import sha
    if case["name"] == "cone":
        z = load_npz("cone_inputs.npz")
        return z["left"], z["right"]
    if case.get("inputs_file") == "cone_inputs.npz":
        z = load_npz("cone_inputs.npz")
        assert sha(z["left"]) == case["sha256_inputs"]["left"]
        return z["left"], z["right"]
    if "file" in case or "inputs_file" in case:
        z = load_npz(case.get("file") or case["inputs_file"])
        if "sha256_inputs" in case:
            assert sha(z["left"]) == case["sha256_inputs"]["left"] and sha(z["right"]) == case["sha256_inputs"]["right"]
        return z["left"], z["right"]
    l, r = oracle.synth_pair(case["w"], case["h"], case["d"], case["seed"])
    assert sha(l) == case["sha256_inputs"]["left"] and sha(r) == case["sha256_inputs"]["right"]
    return l, r
