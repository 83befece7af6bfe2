"""Every caller of the winner-take-all on the planted inputs of tests/wta_classes.py -- needs an MI355X.  Those inputs make the top
index of every layout the winner, put 65535 beside an interior best and take the denominator's clamp on hundreds of pixels
(test_wta_classes_cpu.py has the counts and pins the oracle on them against the reference's own C).  Bit-exact, tolerance 0, against
the CPU oracle: the separate sum / right-view kernels, the fused row kernel plain, storing S (keep_stages), accumulating (a second
match without Reset), in row segments, TIGHT on and off, with the confidence output, in a batch; the fused last sweep; the row-tile
finish; match_both's dual pass; the right reference view; the symmetric census."""
import os
import subprocess
import sys

import numpy as np
import pytest

import confidence_ref as CR
import wta_classes as WC
from oracle.pyoracle import STAGE_NAMES, Oracle
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

NAMES = [f"{s}-{v}" for s, v, _ in WC.INPUTS]
BY_NAME = {f"{s}-{v}": (s, v, seed) for s, v, seed in WC.INPUTS}
MAPS = ("disp_l", "disp_r", "after_lr", "final")
TOPS = [f"{s}-top" for s in WC.TOP_SHAPES]


def stride(p):
    return next(dp for dp in (32, 64, 128, 192, 256, 512) if p.D <= dp)


def instance(monkeypatch, batch=1, **env):
    import soc_project_stereo_matching_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))                                  # read at sgm_create / at the launch
    return S.SGMInstance(0, batch=batch)


def other_view(p):
    """the oracle's stages with the right image as the reference view (a context of its own: the session's oracle stays as it is)"""
    orc = Oracle()
    orc.set_reference_view(True)
    return orc.run(p.left, p.right, p.option)


def check_counts(p, S):
    """the library's own S puts the same number of pixels into every class as the fixture says"""
    import json
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "wta_classes.json")) as f:
        want = json.load(f)["inputs"][p.name]
    got = p.counts(S)
    for v in WC.VIEWS:
        assert got[v] == want["counts"][v], f"{p.name}: {v} view: class counts from the library's S"
        for n in want["planted"][v]:
            assert got[v][n] >= want["floor"]


@pytest.mark.parametrize("path", ["fused", "fused_keep", "separate", "separate_keep"])
@pytest.mark.parametrize("name", NAMES)
def test_single_frame_paths(monkeypatch, name, path):
    p = WC.planted(*BY_NAME[name])
    w, h = p.shape[:2]
    keep = path.endswith("keep")
    i = instance(monkeypatch, SGM_FUSED_WTA=0 if path.startswith("separate") else 1)
    try:
        i.keep_stages(keep)
        assert i.reset(w, h, p.option)
        out = i.match(p.left, p.right)
        assert out is not None
        assert_same(out, p.stages["final"], f"{name} {path}: result")
        for n in (MAPS if keep else ("disp_r",)):
            assert_same(i.read_stage(n), p.stages[n], f"{name} {path}: {n}")
        S = i.read_stage("aggr")                                       # stored, or put together after the fact
        assert_same(S, p.stages["aggr"], f"{name} {path}: aggr")
        if keep:
            check_counts(p, S)
    finally:
        i.close()


@pytest.mark.parametrize("segments", [2, 4])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("288x16_d4-36")])
def test_row_segments(monkeypatch, name, segments):
    """288 columns at a full stride of 32 (D = 32, every lane slot in use; "top": the winner in the last one): the launcher keeps
    four segments (288 / 4 >= 2 x 32), each re-summing dmin + D - 1 columns of its right neighbour"""
    p = WC.planted(*BY_NAME[name])
    w, h = p.shape[:2]
    assert h <= 24 and w // segments >= 2 * stride(p)
    i = instance(monkeypatch, SGM_FUSED_WTA=1, SGM_SUM_SEGMENTS=segments)
    try:
        i.keep_stages(False)
        assert i.reset(w, h, p.option)
        assert_same(i.match(p.left, p.right), p.stages["final"], f"{name} segments={segments}: result")
        assert_same(i.read_stage("disp_r"), p.stages["disp_r"], f"{name} segments={segments}: disp_r")
    finally:
        i.close()


def _tight_child(tight):
    """SGM_SUM_TIGHT is read once per process, at the first fused launch: the inputs of stride 192 / 256 in a process of their own"""
    import soc_project_stereo_matching_amd as S
    assert os.environ["SGM_SUM_TIGHT"] == tight
    for name in NAMES:
        p = WC.planted(*BY_NAME[name])
        if stride(p) not in (192, 256):
            continue
        for keep in (False, True):
            i = S.SGMInstance(0)
            try:
                i.keep_stages(keep)
                assert i.reset(p.shape[0], p.shape[1], p.option)
                assert_same(i.match(p.left, p.right), p.stages["final"], f"{name} tight={tight} keep={keep}: result")
                for n in (MAPS if keep else ("disp_r",)):
                    assert_same(i.read_stage(n), p.stages[n], f"{name} tight={tight} keep={keep}: {n}")
            finally:
                i.close()
    print("tight child ok")


@pytest.mark.parametrize("tight", ["0", "1"])
def test_tight_on_and_off(tight):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SGM_SUM_TIGHT=tight, SGM_FUSED_WTA="1",
               PYTHONPATH=os.pathsep.join([root] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "tight", tight], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tight child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", TOPS + ["64x16_d16-bands", "200x24_d256-p0"])
def test_batch_of_three_distinct_frames(monkeypatch, name, keep):
    s, v, seed = BY_NAME[name]
    ps = [WC.planted(s, v, seed + 0x100 * k) for k in range(3)]
    w, h = ps[0].shape[:2]
    i = instance(monkeypatch, batch=3)
    try:
        i.keep_stages(keep)
        assert i.reset(w, h, ps[0].option)
        out = i.match(np.stack([p.left for p in ps]), np.stack([p.right for p in ps]))
        assert out is not None
        for k, p in enumerate(ps):
            i.select_frame(k)
            assert_same(out[k], p.stages["final"], f"{name} frame {k}: result")
            for n in (MAPS + ("aggr",) if keep else ("disp_r",)):
                assert_same(i.read_stage(n), p.stages[n], f"{name} frame {k}: {n}")
    finally:
        i.close()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_right_reference_view(monkeypatch, name, fused):
    p = WC.planted(*BY_NAME[name])
    want = other_view(p)
    i = instance(monkeypatch, SGM_FUSED_WTA=fused)
    try:
        i.set_reference_view(True)
        i.keep_stages(True)
        assert i.reset(p.shape[0], p.shape[1], p.option)
        assert_same(i.match(p.left, p.right), want["final"], f"{name}: right view: result")
        for n in MAPS:
            assert_same(i.read_stage(n), want[n], f"{name}: right view: {n}")
    finally:
        i.close()


@pytest.mark.parametrize("name", NAMES)
def test_match_both(monkeypatch, name):
    p = WC.planted(*BY_NAME[name])
    w, h = p.shape[:2]
    want_r = other_view(p)["final"]
    i = instance(monkeypatch)
    try:
        i.keep_stages(False)
        assert i.reset(w, h, p.option)
        both = i.match_both(p.left, p.right)
        assert both is not None
        assert_same(both[0], p.stages["final"], f"{name}: both: left")
        assert_same(both[1], want_r, f"{name}: both: right")
        assert i.reset(w, h, p.option)
        assert_same(i.match(p.left, p.right), both[0], f"{name}: single left view")
        i.set_reference_view(True)
        assert i.reset(w, h, p.option)
        assert_same(i.match(p.left, p.right), both[1], f"{name}: single right view")
    finally:
        i.close()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_match_confidence(monkeypatch, name, fused):
    p = WC.planted(*BY_NAME[name])
    dmin = p.shape[2]
    conf = CR.confidence(p.stages["aggr"], dmin, False)[3]
    c = p.classify()["left"]["classes"]
    assert not conf[c["tie"]].any() and not conf[c["none"]].any()     # 0 on ties and where nothing is a candidate
    i = instance(monkeypatch, SGM_FUSED_WTA=fused)
    try:
        i.keep_stages(False)
        assert i.reset(p.shape[0], p.shape[1], p.option)
        got = i.match_confidence(p.left, p.right)
        assert got is not None
        assert_same(got[0], p.stages["final"], f"{name}: confidence: map")
        assert_same(got[1], conf, f"{name}: confidence")
        i.set_reference_view(True)                                     # the right view's confidence: its `none` pixels too
        assert i.reset(p.shape[0], p.shape[1], p.option)
        got = i.match_confidence(p.left, p.right)
        assert got is not None
        assert_same(got[0], other_view(p)["final"], f"{name}: right view: confidence: map")
        assert_same(got[1], CR.confidence(p.stages["aggr"], dmin, True)[3], f"{name}: right view: confidence")
    finally:
        i.close()


@pytest.fixture
def upsum_env(monkeypatch):
    def set_(rows=None, on="1"):
        monkeypatch.setenv("SGM_UPSUM", on)
        if rows is not None:
            monkeypatch.setenv("SGM_UPSUM_ROWS", str(rows))
    return set_


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("150x27_d3-93", "300x24_d128", "140x24_d100"))])
def test_fused_last_sweep(upsum_env, name, batch):
    import soc_project_stereo_matching_amd as S
    upsum_env()
    s, v, seed = BY_NAME[name]
    ps = [WC.planted(s, v, seed + 0x100 * k) for k in range(batch)]
    w, h = ps[0].shape[:2]
    i = S.SGMInstance(0, batch=batch)
    try:
        assert i.reset(w, h, ps[0].option)
        L, R = np.stack([p.left for p in ps]), np.stack([p.right for p in ps])
        out = i.match(L if batch > 1 else L[0], R if batch > 1 else R[0])
        assert out is not None and i.fused_sweep_rows() > 0
        out = out.reshape(batch, h, w)
        for k, p in enumerate(ps):
            i.select_frame(k)
            assert_same(i.read_stage("disp_r"), p.stages["disp_r"], f"{name} frame {k}: disp_r")
            assert_same(out[k], p.stages["final"], f"{name} frame {k}: result")
            assert_same(i.read_stage("aggr"), p.stages["aggr"], f"{name} frame {k}: S after the fact")
    finally:
        i.close()


@pytest.mark.parametrize("name", ["40x45_d8-top", "40x45_d8-p0", "150x27_d3-93-top", "260x24_d192-top"])
def test_three_row_tiles_in_one_process(name):
    import torch
    import soc_project_stereo_matching_amd as S
    from soc_project_stereo_matching_amd.tiling import DeviceTileEngine, match_tiled_in_process, tile_rows
    p = WC.planted(*BY_NAME[name])
    w, h = p.shape[:2]
    engines = []
    try:
        for rows in tile_rows(h, 3):
            e = DeviceTileEngine.__new__(DeviceTileEngine)
            e.torch, e.dev = torch, torch.device("cuda", 0)
            e.w, e.h, e.rows, e.option = w, h, rows, p.option
            e.inst = S.SGMInstance(0)
            engines.append(e)
            assert e.inst.set_rows(*rows) and e.inst.reset(w, h, p.option)
            e.disp = torch.empty((h, w), dtype=torch.float32, device=e.dev)
            e.nbytes = e.inst.tile_boundary_bytes()
        got = match_tiled_in_process(engines, torch.from_numpy(p.left.copy()).cuda(), torch.from_numpy(p.right.copy()).cuda())
        assert_same(got.cpu().numpy(), p.stages["final"], f"{name}: three row tiles")
        for e in engines:
            r0, r1 = e.rows
            assert_same(e.inst.read_stage("aggr")[r0:r1], p.stages["aggr"][r0:r1], f"{name}: S rows {r0}:{r1}")
    finally:
        for e in engines:
            e.inst.close()


def test_symmetric_census_7x7(oracle, monkeypatch):
    import census_sym_ref as CS
    p = WC.planted(*BY_NAME["140x24_d100-top"])
    want = CS.pipeline(oracle, p.left, p.right, p.option, 7, 7)
    assert WC.counts(want["aggr"], p.D, 0)["left"]["last"] >= WC.floor(*p.shape[:2])
    i = instance(monkeypatch)
    try:
        assert i.set_census_kind(1) and i.set_census_window(7, 7)
        i.keep_stages(True)
        assert i.reset(p.shape[0], p.shape[1], p.option)
        assert_same(i.match(p.left, p.right), want["final"], "symmetric 7x7: result")
        for n in MAPS + ("aggr",):
            assert_same(i.read_stage(n), want[n], f"symmetric 7x7: {n}")
    finally:
        i.close()


@pytest.mark.parametrize("mode", ["fused", "fused_keep", "separate"])
@pytest.mark.parametrize("name", TOPS + ["64x16_d16-p0", "200x24_d256-bands", "90x24_d512-p0"])
def test_second_match_without_reset(monkeypatch, name, mode):
    """Q14: the accumulating variants of the sum kernels, on S = one planted frame's sums + another's"""
    s, v, seed = BY_NAME[name]
    a, b = WC.planted(s, v, seed), WC.planted(s, v, seed + 0x100)
    w, h = a.shape[:2]
    orc = Oracle()
    assert orc.reset(w, h, a.option)
    first = orc.match(a.left, a.right)
    second = orc.match(b.left, b.right)
    want = {n: orc.stage(n) for n in STAGE_NAMES}
    if name.endswith("-top"):                                          # the sum of two planted frames still has the top index win
        c = WC.counts(want["aggr"], a.D, a.shape[2], a.unique, a.option.uniqueness_ratio)
        assert min(c["left"]["last"], c["right"]["last"], c["right"]["edge_cost"], c["right"]["flat"]) >= WC.floor(w, h), c
    i = instance(monkeypatch, SGM_FUSED_WTA=0 if mode == "separate" else 1)
    try:
        i.keep_stages(mode != "fused")
        assert i.reset(w, h, a.option)
        assert_same(i.match(a.left, a.right), first, f"{name} {mode}: first")
        assert_same(i.match(b.left, b.right), second, f"{name} {mode}: second (no reset)")
        for n in (("disp_r", "aggr") if mode == "fused" else MAPS + ("aggr",)):
            assert_same(i.read_stage(n), want[n], f"{name} {mode}: second: {n}")
    finally:
        i.close()


@pytest.mark.parametrize("mode", ["fused", "fused_keep", "separate"])
@pytest.mark.parametrize("name", list(WC.Q14_INPUTS))
def test_q14_planted_sequences(monkeypatch, name, mode):
    """Some sixty matches without Reset (tests/q14_deep.py's frames): S past 32768, where the LEFT view takes the clamp of the
    denominator on more pixels than the floor (test_wta_classes_cpu.py).  Every final map, and after the last match the stages
    and the class counts from the library's own S."""
    import json
    from conftest import GOLDEN
    p = WC.q14_planted(name)
    w, h = p.shape[:2]
    i = instance(monkeypatch, SGM_FUSED_WTA=0 if mode == "separate" else 1)
    try:
        i.keep_stages(mode != "fused")
        assert i.reset(w, h, p.option)
        for k, (l, r) in enumerate(p.frames):
            assert_same(i.match(l, r), p.finals[k], f"{name} {mode}: match {k}")
        for n in (("disp_r",) if mode == "fused" else WC.Q14_STAGES[1:]):
            assert_same(i.read_stage(n), p.stages[n], f"{name} {mode}: {n}")
        S = i.read_stage("aggr")
        assert_same(S, p.stages["aggr"], f"{name} {mode}: aggr")
        with open(os.path.join(GOLDEN, "wta_classes.json")) as f:
            want = json.load(f)["inputs"][name]
        got = p.counts(S)
        assert got == want["counts"] and got["left"]["flat"] >= want["floor"]
    finally:
        i.close()


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "tight":
    _tight_child(sys.argv[2])
