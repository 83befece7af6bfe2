"""Matching confidence (include/sgm_mi355x.h, SGM_MatchConfidence) on the CPU: the numpy restatement tests/confidence_ref.py
tied to the reference's own winner-take-all arithmetic through the oracle's digest-pinned stages, hand-made cost volumes, the
exported interface, and the host logic on the stand-in device.  Parity unpinned by the reference: the reference computes
m1 / m2 but never exposes them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import confidence_ref as R
import standin
from conftest import ROOT, case_inputs, option_from_dict

CPU_CASES = ["cone", "t24x16_d8", "t70x33_d16", "t20x31_d8_tall", "t40x24_d16_dmin3", "t33x33_d12_square", "t64x20_d40",
             "v_default", "v_no_unique", "v_no_lr", "v_p1_0_p2_0", "v_p_big", "v_ratio_095", "c1_synth_450x375_d64",
             "d256_400x48", "d192_300x60"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement against the oracle's stages -------------------------------------------------------------------

@pytest.mark.parametrize("name", CPU_CASES)
def test_restatement_reproduces_the_reference_wta(oracle, golden_cases, name):
    """m1 / m2 / d1 of the restatement, fed through the reference's WTA formulas, give the oracle's disp_l and disp_r stages bit
    for bit (uniqueness on and off, both views); aggr is the digest-pinned stage 3."""
    case = golden_cases[name]
    left, right = case_inputs(case, oracle)
    for unique in (True, False):
        opt = option_from_dict(case["option"])
        opt.is_check_unique = unique
        opt.is_check_lr = True                                  # the oracle makes the right view's map for the LR check
        st = oracle.run(left, right, opt)
        S = st["aggr"]
        for right_view, stage in ((False, "disp_l"), (True, "disp_r")):
            m1, m2, d1, conf = R.confidence(S, opt.min_disparity, right_view)
            got = R.wta(S, m1, m2, d1, opt.min_disparity, opt.max_disparity, unique, opt.uniqueness_ratio, right_view)
            assert np.array_equal(bits(got), bits(st[stage])), (name, unique, stage)
            assert conf.dtype == np.uint16 and conf.shape == S.shape[:2]


def test_confidence_is_independent_of_the_uniqueness_options(oracle, golden_cases):
    case = golden_cases["t70x33_d16"]
    left, right = case_inputs(case, oracle)
    confs = []
    for unique, ratio in ((True, 0.99), (False, 0.99), (True, 0.5)):
        opt = option_from_dict(case["option"])
        opt.is_check_unique, opt.uniqueness_ratio = unique, ratio
        confs.append(R.confidence(oracle.run(left, right, opt)["aggr"])[3])
    assert all(np.array_equal(confs[0], c) for c in confs[1:])
    assert (confs[0] > 0).any()


# ---- hand-made volumes -----------------------------------------------------------------------------------------------

def vol(costs):
    return np.array(costs, np.uint16).reshape(1, 1, -1)


def test_tie_for_the_best_cost_gives_zero():
    m1, m2, d1, conf = R.confidence(vol([9, 4, 7, 4, 8]))
    assert (m1[0, 0], m2[0, 0], d1[0, 0], conf[0, 0]) == (4, 4, 1, 0)


def test_formula_floor_and_m1_zero():
    m1, m2, d1, conf = R.confidence(vol([0, 5, 3]))
    assert (m1[0, 0], m2[0, 0], d1[0, 0], conf[0, 0]) == (0, 3, 0, 65535)     # m1 = 0: full confidence
    _, _, _, conf = R.confidence(vol([10, 7, 30]))
    assert conf[0, 0] == (3 * 65535) // 10                                       # floor
    _, _, _, conf = R.confidence(vol([0, 0, 3]))
    assert conf[0, 0] == 0                                                       # m2 == 0


def test_single_disparity():
    m1, m2, d1, conf = R.confidence(vol([7]))
    assert (m1[0, 0], m2[0, 0], d1[0, 0]) == (7, 65535, 0)
    assert conf[0, 0] == ((65535 - 7) * 65535) // 65535
    assert R.confidence(vol([0]))[3][0, 0] == 65535


def test_no_candidate_gives_zero():
    m1, m2, d1, conf = R.confidence(vol([65535, 65535]))
    assert (m1[0, 0], m2[0, 0], d1[0, 0], conf[0, 0]) == (65535, 65535, -1, 0)


def test_right_view_columns_off_the_image():
    # W = 3, D = 3, dmin = 1: right pixel x reads S[y][x + 1 + k][k]; x = 2 has no column at all, x = 1 only k = 0
    S = np.zeros((1, 3, 3), np.uint16)
    S[0, :, 0] = [50, 20, 40]
    S[0, :, 1] = [60, 70, 10]
    S[0, :, 2] = [90, 90, 30]
    m1, m2, d1, conf = R.confidence(S, dmin=1, right=True)
    assert list(m1[0]) == [10, 40, 65535] and list(d1[0]) == [1, 0, -1]
    assert list(m2[0]) == [20, 65535, 65535]
    assert list(conf[0]) == [(10 * 65535) // 20, ((65535 - 40) * 65535) // 65535, 0]
    # the left view of the same volume ignores dmin
    m1, _, d1, _ = R.confidence(S, dmin=1, right=False)
    assert list(m1[0]) == [50, 20, 10] and list(d1[0]) == [0, 0, 1]


# ---- the exported interface ------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as f:
        h = f.read()
    for decl in (r"bool\s+SGM_MatchConfidence\(const uint8_t\* img_left, const uint8_t\* img_right, float\* disp_left, uint16_t\* conf\)",
                 r"bool\s+sgm_match_confidence\(sgm_instance\* s,",
                 r"bool\s+sgm_match_confidence_async\(sgm_instance\* s,",
                 r"bool\s+sgm_match_confidence_device\(sgm_instance\* s,"):
        assert re.search(decl, h), decl
    assert "parity unpinned by the reference" in h and "(m2 - m1) * 65535u) / m2" in h


def test_library_exports_confidence():
    import soc_project_stereo_matching_amd as S
    path = S.library_path()
    if not os.path.exists(path):
        pytest.skip("libsgm_mi355x.so not built (no hipcc here)")
    lib = S.load_library()
    for sym in ("sgm_match_confidence", "sgm_match_confidence_async", "sgm_match_confidence_device", "SGM_MatchConfidence",
                "sgmd_sum_wta_conf", "sgmd_sum_wta_lr_conf", "sgmd_wta_right_conf"):
        assert hasattr(lib, sym), sym
    assert callable(getattr(S.SGM, "match_confidence", None))
    for m in ("match_confidence", "match_confidence_async", "match_confidence_device"):
        assert callable(getattr(S.SGMInstance, m, None)), m


# ---- host logic on the stand-in device ---------------------------------------------------------------------------------

CONF = ("sum_wta_conf", "sum_wta_lr_conf", "wta_right_conf")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return standin.build(tmp_path_factory.mktemp("confstub"))


@pytest.fixture(scope="module")
def host_old(tmp_path_factory):
    return standin.build(tmp_path_factory.mktemp("confstub"), without=("conf", "refine", "both"))


def full_log(L):
    return [(e.name, e.arg) for e in standin.log(L)]


launches = standin.launches


def conf_calls(L):
    return standin.calls(L, *CONF)


def clear(L):
    L.stub_clear()


class Frame:
    def __init__(self, w=48, h=20, b=1):
        self.left = np.zeros((b, h, w), np.uint8)
        self.right = np.zeros((b, h, w), np.uint8)
        self.out = np.zeros((b, h, w), np.float32)
        self.conf = np.zeros((b, h, w), np.uint16)

    def args(self):
        return self.left.ctypes.data, self.right.ctypes.data, self.out.ctypes.data

    def cargs(self):
        return self.args() + (self.conf.ctypes.data,)


def fresh(L, d=16, w=48, h=20, batch=1, right_view=False, **kw):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    if batch > 1:
        assert L.sgm_set_batch(s, batch)
    L.sgm_set_reference_view(s, 1 if right_view else 0)
    opt = S.default_option(d, **kw)
    assert L.sgm_reset(s, w, h, C.byref(opt))
    clear(L)
    return s, opt


@pytest.mark.parametrize("d", [16, 300], ids=["fused", "separate"])
@pytest.mark.parametrize("right_view", [False, True], ids=["left", "right"])
def test_each_path_stores_the_reference_view(host, d, right_view):
    L = host
    s, _ = fresh(L, d=d, right_view=right_view)
    f = Frame()
    assert L.sgm_match_confidence(s, *f.cargs())
    names = [n for n, _ in launches(L)]
    if d == 16:
        assert names[:3] == ["census", "aggregate", "sum_wta_lr_conf"]
        assert conf_calls(L)[0].arg == (4 | (8 if right_view else 0))          # do_right, conf_right
    elif right_view:
        assert names[:4] == ["census", "aggregate", "sum_wta", "wta_right_conf"]
    else:
        assert names[:4] == ["census", "aggregate", "sum_wta_conf", "wta_right"]
    assert len(conf_calls(L)) == 1
    L.sgm_destroy(s)


def test_plain_match_is_unchanged_after_a_confidence_match(host):
    L = host
    for d, right_view in ((16, False), (16, True), (300, False)):
        f = Frame()
        s, _ = fresh(L, d=d, right_view=right_view)
        assert L.sgm_match(s, *f.args())
        # launches and copies (a fresh instance of the separate path also allocates S at its first match)
        plain_fresh = launches(L, drop=("sync", "alloc", "memset"))
        L.sgm_destroy(s)
        s, _ = fresh(L, d=d, right_view=right_view)
        assert L.sgm_match_confidence(s, *f.cargs())
        assert L.sgm_reset(s, 48, 20, C.byref(_))
        clear(L)
        assert L.sgm_match(s, *f.args())
        assert launches(L, drop=("sync", "alloc", "memset")) == plain_fresh and conf_calls(L) == []
        L.sgm_destroy(s)


def test_device_form_writes_the_callers_map(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    assert L.sgm_match_confidence_device(s, *f.cargs())
    assert conf_calls(L)[0].a == f.conf.ctypes.data
    assert "d2h" not in [n for n, _ in full_log(L)]
    L.sgm_destroy(s)


def test_host_form_copies_the_map_back(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    assert L.sgm_match_confidence_async(s, *f.cargs())
    assert L.sgm_match_wait(s)
    assert conf_calls(L)[0].a not in (None, f.conf.ctypes.data)             # the instance's device staging map
    assert [n for n, _ in full_log(L)].count("d2h") >= 2                     # disparity + confidence
    L.sgm_destroy(s)


def test_confidence_never_takes_the_fused_last_sweep(host, monkeypatch):
    L = host
    monkeypatch.setenv("SGM_UPSUM", "1")
    s, _ = fresh(L, d=128, w=200, h=30, batch=2)
    f = Frame(w=200, h=30, b=2)
    assert L.sgm_match_device(s, *f.args())
    assert L.sgm_fused_sweep_rows(s) == 3 and "upsum" in [n for n, _ in launches(L)]
    assert L.sgm_reset(s, 200, 30, C.byref(_))
    clear(L)
    assert L.sgm_match_confidence_device(s, *f.cargs())
    assert L.sgm_fused_sweep_rows(s) == 0
    got = launches(L)
    assert "upsum" not in [n for n, _ in got] and ("aggregate", 0xFF) in got and "sum_wta_lr_conf" in [n for n, _ in got]
    # ... and the plain match after it runs fused again
    assert L.sgm_reset(s, 200, 30, C.byref(_))
    clear(L)
    assert L.sgm_match_device(s, *f.args())
    assert L.sgm_fused_sweep_rows(s) == 3
    L.sgm_destroy(s)


def test_null_conf_returns_false_and_queues_nothing(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    for fn in (L.sgm_match_confidence, L.sgm_match_confidence_async, L.sgm_match_confidence_device):
        clear(L)
        assert not fn(s, *f.args(), None)
        assert full_log(L) == []
    L.sgm_destroy(s)


def test_row_tile_mode_refuses(host):
    L = host
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert L.sgm_set_rows(s, 0, 10)
    opt = S.default_option(16)
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    f = Frame()
    for fn in (L.sgm_match_confidence, L.sgm_match_confidence_device):
        assert not fn(s, *f.cargs())
    assert [n for n, _ in full_log(L) if n not in ("sync",)] == []
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_old):
    L = host_old
    s, _ = fresh(L)
    f = Frame()
    for fn in (L.sgm_match_confidence, L.sgm_match_confidence_async, L.sgm_match_confidence_device):
        L.stub_clear()
        assert not fn(s, *f.cargs())
        assert [n for n, _ in full_log(L) if n != "sync"] == []
    L.stub_clear()
    assert L.sgm_match(s, *f.args())                                         # the plain match is untouched
    L.sgm_destroy(s)
