"""Both views' maps from one match (include/sgm_mi355x.h, SGM_MatchBoth) on the CPU: the exported interface, the host restatement
of the both-views post pass by the oracle's stages, the host logic on the stand-in device (tests/stub_device.c), and the host
under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import standin
from conftest import ROOT, case_inputs, option_from_dict

TINY_CASES = ["t24x16_d8", "t70x33_d16", "t20x31_d8_tall", "t40x24_d16_dmin3", "t33x33_d12_square", "t64x20_d40"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the post pass of both views, restated with the oracle's stages --------------------------------------------------------

def lrcheck_right(oracle, dr, dl, thres):
    dr = dr.copy()
    h, w = dr.shape
    oracle.lib.sgmo_lrcheck_right.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    oracle.lib.sgmo_lrcheck_right.restype = None
    oracle.lib.sgmo_lrcheck_right(dr.ctypes.data, np.ascontiguousarray(dl).ctypes.data, w, h, thres)
    return dr


@pytest.mark.parametrize("name", TINY_CASES)
def test_chaining_the_oracles_stages_reproduces_both_final_maps(oracle, golden_cases, name):
    """Both checks read the RAW maps (copies of stages 4 and 5), then speckle removal and the median per map: that is
    oracle.run(...)[final] of either reference view, bit for bit -- what the dual LR check kernel and the batched post pass do."""
    case = golden_cases[name]
    left, right = case_inputs(case, oracle)
    opt = option_from_dict(case["option"])
    opt.is_check_lr = True
    final = {}
    try:
        for view in (False, True):
            oracle.set_reference_view(view)
            final[view] = oracle.run(left, right, opt)
    finally:
        oracle.set_reference_view(False)
    raw_l, raw_r = final[False]["disp_l"].copy(), final[False]["disp_r"].copy()
    assert np.array_equal(bits(raw_r), bits(final[True]["disp_r"]))
    chk_l = oracle.lrcheck(raw_l, raw_r, opt.lrcheck_thres)
    chk_r = lrcheck_right(oracle, raw_r, raw_l, opt.lrcheck_thres)
    for view, m in ((False, chk_l), (True, chk_r)):
        assert np.array_equal(bits(m), bits(final[view]["after_lr"])), (name, view, "after_lr")
        if opt.is_remove_speckles:
            m = oracle.remove_speckles(m, opt.min_speckle_area)
        assert np.array_equal(bits(oracle.median(m)), bits(final[view]["final"])), (name, view, "final")


# ---- the exported interface ---------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as f:
        h = f.read()
    for decl in (r"bool\s+SGM_MatchBoth\(const uint8_t\* img_left, const uint8_t\* img_right, float\* disp_left, float\* disp_right\)",
                 r"bool\s+sgm_match_both\(sgm_instance\* s,", r"bool\s+sgm_match_both_async\(sgm_instance\* s,",
                 r"bool\s+sgm_match_both_device\(sgm_instance\* s,", r"bool\s+sgm_depth_from_both\(sgm_instance\* s,"):
        assert re.search(decl, h), decl
    assert "parity unpinned by the reference" in h and "26 right view after the LR check" in h


def test_library_exports_both():
    import soc_project_stereo_matching_amd as S
    if not os.path.exists(S.library_path()):
        pytest.skip("libsgm_mi355x.so not built (no hipcc here)")
    lib = S.load_library()
    for sym in ("sgm_match_both", "sgm_match_both_async", "sgm_match_both_device", "SGM_MatchBoth", "sgm_depth_from_both",
                "sgmd_lrcheck_both", "sgmd_depth_both"):
        assert hasattr(lib, sym), sym
    assert callable(getattr(S.SGM, "match_both", None))
    for m in ("match_both", "match_both_async", "match_both_device", "depth_from_both"):
        assert callable(getattr(S.SGMInstance, m, None)), m


# ---- host logic on the stand-in device ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return standin.build(tmp_path_factory.mktemp("bothstub"))


@pytest.fixture(scope="module")
def host_old(tmp_path_factory):
    return standin.build(tmp_path_factory.mktemp("bothstub"), without=("conf", "refine", "both"))


def full_log(L):
    return [(e.name, e.arg) for e in standin.log(L)]


launches = standin.launches


def both_calls(L):
    """the both-views launches: a, b = their left / right map"""
    return standin.calls(L, "lrcheck_both", "depth_both")


def clear(L):
    L.stub_clear()


def nothing_queued(L):
    return [n for n, _ in full_log(L) if n != "sync"] == []


class Frame:
    def __init__(self, w=48, h=20, b=1):
        self.left = np.zeros((b, h, w), np.uint8)
        self.right = np.zeros((b, h, w), np.uint8)
        self.out = np.full((b, h, w), -1, np.float32)
        self.out_r = np.full((b, h, w), -1, np.float32)

    def args(self):
        return self.left.ctypes.data, self.right.ctypes.data, self.out.ctypes.data

    def bargs(self):
        return self.args() + (self.out_r.ctypes.data,)


def fresh(L, d=16, w=48, h=20, batch=1, **kw):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    if batch > 1:
        assert L.sgm_set_batch(s, batch)
    opt = S.default_option(d, **kw)
    assert L.sgm_reset(s, w, h, C.byref(opt))
    clear(L)
    return s, opt


@pytest.mark.parametrize("d", [16, 300], ids=["fused", "separate"])
@pytest.mark.parametrize("view", [0, 1])
def test_one_cost_sum_feeds_one_post_pass_over_both_views(host, d, view):
    L = host
    s, _ = fresh(L, d=d)
    L.sgm_set_reference_view(s, view)                            # neither read nor changed
    f = Frame()
    assert L.sgm_match_both(s, *f.bargs())
    names = [n for n, _ in launches(L)]
    head = ["census", "aggregate", "sum_wta_lr"] if d == 16 else ["census", "aggregate", "sum_wta", "wta_right"]
    assert names == head + ["lrcheck_both", "speckle", "median"]
    assert both_calls(L)[0].arg == (1 | (1 << 8))                 # the check is on, on B = 1 frames
    # the two outputs are the halves of one batch of 2 B maps
    assert both_calls(L)[0].b - both_calls(L)[0].a == f.out.nbytes
    assert (f.out == 1.0).all() and (f.out_r == 2.0).all()
    L.sgm_destroy(s)


def test_lr_check_off_still_finishes_both_maps(host):
    L = host
    s, _ = fresh(L, is_check_lr=False)
    f = Frame()
    assert L.sgm_match_both(s, *f.bargs())
    assert [n for n, _ in launches(L)] == ["census", "aggregate", "sum_wta_lr", "lrcheck_both", "speckle", "median"]
    assert both_calls(L)[0].arg == (0 | (1 << 8))                 # plain copies of the raw maps
    L.sgm_destroy(s)


def test_buffers_come_with_the_first_both_call_and_only_then(host):
    L = host
    f = Frame(b=2)
    s, opt = fresh(L, batch=2)
    assert L.sgm_match(s, *f.args())
    plain_first = full_log(L)
    assert not any(n == "alloc" for n, _ in plain_first)          # a plain match allocates nothing after initialize
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    assert L.sgm_match_both(s, *f.bargs())
    allocs = [a for n, a in full_log(L) if n == "alloc"]
    px4 = f.out.nbytes
    # the raw left map, the 2 B finished maps, three speckle scratch maps of 2 B maps, the median scratch (the stand-in's size)
    assert sorted(allocs) == sorted([px4 >> 10] + [2 * px4 >> 10] * 4 + [48 * 20 * 4 >> 10])
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    assert L.sgm_match_both(s, *f.bargs())
    assert not any(n == "alloc" for n, _ in full_log(L))          # grow-only: nothing the second time
    # ... and a plain match afterwards launches exactly what it did before
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    assert L.sgm_match(s, *f.args())
    assert full_log(L) == plain_first and both_calls(L) == []
    L.sgm_destroy(s)


def test_plain_match_log_is_the_same_with_and_without_the_launchers(host, host_old):
    logs = []
    for L in (host, host_old):
        s, _ = fresh(L)
        f = Frame()
        assert L.sgm_match(s, *f.args()) and L.sgm_match_device(s, *f.args())
        logs.append(full_log(L))
        L.sgm_destroy(s)
    assert logs[0] == logs[1]


def test_null_outputs_return_false_and_queue_nothing(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    for fn in (L.sgm_match_both, L.sgm_match_both_async, L.sgm_match_both_device):
        for args in ((f.left.ctypes.data, f.right.ctypes.data, f.out.ctypes.data, None),
                     (f.left.ctypes.data, f.right.ctypes.data, None, f.out_r.ctypes.data),
                     (None, f.right.ctypes.data, f.out.ctypes.data, f.out_r.ctypes.data)):
            clear(L)
            assert not fn(s, *args)
            assert full_log(L) == []
    L.sgm_destroy(s)


def test_row_tile_mode_refuses(host):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    assert L.sgm_set_rows(s, 0, 10)
    opt = S.default_option(16)
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    f = Frame()
    for fn in (L.sgm_match_both, L.sgm_match_both_async, L.sgm_match_both_device):
        assert not fn(s, *f.bargs())
    assert nothing_queued(L)
    L.sgm_destroy(s)


@pytest.mark.parametrize("what", ["fill", "refine"])
def test_hole_filling_and_refinement_refuse(host, what):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    assert L.sgm_set_fill_holes(s, 1) if what == "fill" else L.sgm_set_refine(s, 1, 16.0, 1.5, 1, 0)
    opt = S.default_option(16)
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    f = Frame()
    for fn in (L.sgm_match_both, L.sgm_match_both_async, L.sgm_match_both_device):
        assert not fn(s, *f.bargs())
    assert nothing_queued(L)
    assert L.sgm_match(s, *f.args())                              # the single-view match goes on as before
    # switched off again (next reset): both views are back
    assert L.sgm_set_fill_holes(s, 0) and L.sgm_set_refine(s, 0, 0, 0, 0, 0) and L.sgm_reset(s, 48, 20, C.byref(opt))
    assert L.sgm_match_both(s, *f.bargs())
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_and_refuses(host_old):
    L = host_old
    s, _ = fresh(L)
    f = Frame()
    for fn in (L.sgm_match_both, L.sgm_match_both_async, L.sgm_match_both_device):
        L.stub_clear()
        assert not fn(s, *f.bargs())
        assert nothing_queued(L)
    assert not L.sgm_depth_from_both(s, f.out.ctypes.data, f.out_r.ctypes.data, f.out.size, 1.0, 1.0, 1.0, 0.0, f.out.ctypes.data)
    L.stub_clear()
    assert L.sgm_match(s, *f.args())                              # the plain match is untouched
    L.sgm_destroy(s)


def test_async_hands_over_two_maps_at_the_wait(host):
    L = host
    s, opt = fresh(L, batch=2)
    f = Frame(b=2)
    assert L.sgm_match_both_async(s, *f.bargs())
    # pageable buffers: staged, nothing in the caller's maps before the wait
    assert (f.out == -1).all() and (f.out_r == -1).all()
    assert [a for n, a in full_log(L) if n == "d2h"] == [f.out.nbytes, f.out_r.nbytes]
    assert L.sgm_match_wait(s)
    assert (f.out == 1.0).all() and (f.out_r == 2.0).all()
    # a second wait hands nothing over again
    f.out_r.fill(-1)
    assert L.sgm_match_wait(s) and (f.out_r == -1).all()
    # the next entry point waits by itself
    assert L.sgm_reset(s, 48, 20, C.byref(opt)) and L.sgm_match_both_async(s, *f.bargs())
    g = Frame(b=2)
    assert L.sgm_match_async(s, *g.args())
    assert (f.out_r == 2.0).all()
    assert L.sgm_match_wait(s)
    L.sgm_destroy(s)


@pytest.mark.parametrize("pin_left,pin_right", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["pinned-pinned", "pinned-staged", "staged-pinned", "staged-staged"])
def test_pinned_and_staged_outputs_each_go_their_own_way(host, pin_left, pin_right):
    """A page-locked output (sgm_host_alloc) is written by the device copy itself and never touched by sgm_match_wait; a pageable one
    is staged and handed over at the wait.  The two outputs decide independently; the right map's page-locked staging is allocated
    only when the right output needs it."""
    L = host
    s, opt = fresh(L, batch=2)
    f = Frame(b=2)
    try:
        L.stub_set_pinned(0, f.out.ctypes.data if pin_left else None)
        L.stub_set_pinned(1, f.out_r.ctypes.data if pin_right else None)
        before = L.stub_alloc_count()
        assert L.sgm_match_both_async(s, *f.bargs())
        # six device buffers at the first call, and the right map's page-locked staging exactly when that map is pageable
        assert L.stub_alloc_count() - before == 6 + (0 if pin_right else 1)
        assert [a for n, a in full_log(L) if n == "d2h"] == [f.out.nbytes, f.out_r.nbytes]
        # the stand-in copies at once: a page-locked output already holds its map, a pageable one nothing yet
        assert (f.out == (1.0 if pin_left else -1.0)).all() and (f.out_r == (2.0 if pin_right else -1.0)).all()
        # what the wait hands over: the staged map(s) only -- a mark in a page-locked output survives it
        if pin_left:
            f.out[0, 0, 0] = 7.0
        if pin_right:
            f.out_r[0, 0, 0] = 7.0
        assert L.sgm_match_wait(s)
        want_l, want_r = np.full_like(f.out, 1.0), np.full_like(f.out_r, 2.0)
        if pin_left:
            want_l[0, 0, 0] = 7.0
        if pin_right:
            want_r[0, 0, 0] = 7.0
        assert np.array_equal(f.out, want_l) and np.array_equal(f.out_r, want_r)
        # the same instance with the roles swapped: nothing of the first hand-over is left behind
        g = Frame(b=2)
        L.stub_set_pinned(0, g.out.ctypes.data if not pin_left else None)
        L.stub_set_pinned(1, g.out_r.ctypes.data if not pin_right else None)
        assert L.sgm_reset(s, 48, 20, C.byref(opt)) and L.sgm_match_both_async(s, *g.bargs())
        assert (g.out == (-1.0 if pin_left else 1.0)).all() and (g.out_r == (-1.0 if pin_right else 2.0)).all()
        f.out.fill(-5), f.out_r.fill(-5)
        assert L.sgm_match_wait(s)
        assert (g.out == 1.0).all() and (g.out_r == 2.0).all()
        assert (f.out == -5).all() and (f.out_r == -5).all()      # the earlier call's buffers are no longer written
    finally:
        L.stub_set_pinned(0, None)
        L.stub_set_pinned(1, None)
        L.sgm_destroy(s)


def test_pinned_inputs_are_uploaded_in_place(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    try:
        f.left.fill(9)
        L.stub_set_pinned(0, f.left.ctypes.data)
        assert L.sgm_match_both_async(s, *f.bargs()) and L.sgm_match_wait(s)
        assert (f.out == 1.0).all() and (f.out_r == 2.0).all()
    finally:
        L.stub_set_pinned(0, None)
        L.sgm_destroy(s)


def test_device_form_copies_into_the_callers_maps_and_nothing_to_the_host(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    assert L.sgm_match_both_device(s, *f.bargs())
    log = full_log(L)
    assert "d2h" not in [n for n, _ in log] and "h2d" not in [n for n, _ in log]
    assert [a for n, a in log if n == "d2d"][-2:] == [f.out.nbytes, f.out_r.nbytes]
    assert (f.out == 1.0).all() and (f.out_r == 2.0).all()      # ("device" memory is host memory on the stand-in)
    L.sgm_destroy(s)


def test_both_never_takes_the_fused_last_sweep(host, monkeypatch):
    L = host
    monkeypatch.setenv("SGM_UPSUM", "1")
    s, opt = fresh(L, d=128, w=200, h=30, batch=2)
    f = Frame(w=200, h=30, b=2)
    assert L.sgm_match_device(s, *f.args()) and L.sgm_fused_sweep_rows(s) == 3
    assert L.sgm_reset(s, 200, 30, C.byref(opt))
    clear(L)
    assert L.sgm_match_both_device(s, *f.bargs())
    got = launches(L)
    assert L.sgm_fused_sweep_rows(s) == 0 and "upsum" not in [n for n, _ in got] and ("aggregate", 0xFF) in got
    assert L.sgm_reset(s, 200, 30, C.byref(opt)) and L.sgm_match_device(s, *f.args()) and L.sgm_fused_sweep_rows(s) == 3
    L.sgm_destroy(s)


def test_q14_accumulates_once_per_call(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    assert L.sgm_match_both(s, *f.bargs()) and L.sgm_match_both(s, *f.bargs())
    sums = [(n, a) for n, a in launches(L) if n.startswith("sum_wta")]
    # the second call: the pending sum of the first goes to S (sum_wta), then ONE accumulating cost sum
    assert sums == [("sum_wta_lr", 0), ("sum_wta", 0), ("sum_wta_lr", 1)]
    L.sgm_destroy(s)


def test_overlap_post_runs_the_both_views_post_pass_behind_the_event(host):
    L = host
    s, opt = fresh(L)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, 48, 20, C.byref(opt))
    clear(L)
    f = Frame()
    assert L.sgm_match_both_device(s, *f.bargs())
    names = [n for n, _ in launches(L, drop=("sync", "alloc", "memset"))]
    assert names == ["census", "aggregate", "sum_wta_lr", "event_record", "wait_event", "lrcheck_both", "speckle", "median", "d2d", "d2d",
                     "event_record"]
    L.sgm_destroy(s)


def test_a_refused_launch_ends_the_match(host):
    L = host
    s, opt = fresh(L)
    f = Frame()
    L.stub_fail_at(b"speckle", 0)
    assert not L.sgm_match_both(s, *f.bargs())
    assert "median" not in [n for n, _ in launches(L)]
    assert L.sgm_reset(s, 48, 20, C.byref(opt)) and L.sgm_match_both(s, *f.bargs())
    L.sgm_destroy(s)


def test_right_view_stages_belong_to_the_last_completed_both_match(host):
    L = host
    s, opt = fresh(L)
    f = Frame()
    buf = np.zeros((20, 48), np.float32)

    def stage(which):
        return L.sgm_read_stage(s, which, buf.ctypes.data, buf.nbytes)

    L.sgm_keep_stages(s, 1)
    assert L.sgm_match_both(s, *f.bargs())
    assert [stage(w) for w in (26, 27, 28)] == [buf.nbytes] * 3
    # a both-match that ran WITHOUT kept stages leaves no snapshots of its own, whatever an earlier one left in the buffer
    L.sgm_keep_stages(s, 0)
    assert L.sgm_reset(s, 48, 20, C.byref(opt)) and L.sgm_match_both(s, *f.bargs())
    L.sgm_keep_stages(s, 1)
    assert [stage(w) for w in (26, 27, 28)] == [0, 0, buf.nbytes]
    # a both-match that was abandoned half way has no finished right map
    assert L.sgm_reset(s, 48, 20, C.byref(opt))
    L.stub_fail_at(b"median", 0)
    assert not L.sgm_match_both(s, *f.bargs())
    assert [stage(w) for w in (26, 27, 28)] == [0, 0, 0]
    assert L.sgm_reset(s, 48, 20, C.byref(opt)) and L.sgm_match_both(s, *f.bargs())
    assert [stage(w) for w in (26, 27, 28)] == [buf.nbytes] * 3
    assert L.sgm_match(s, *f.args()) and [stage(w) for w in (26, 27, 28)] == [0, 0, 0]
    L.sgm_destroy(s)


def test_depth_from_both_is_one_launch(host):
    L = host
    s, _ = fresh(L)
    f = Frame()
    assert L.sgm_depth_from_both(s, f.out.ctypes.data, f.out_r.ctypes.data, f.out.size, 1000.0, 1001.0, 100.0, 0.0, f.out.ctypes.data)
    assert [(e.name, e.arg) for e in both_calls(L)] == [("depth_both", f.out.size)]
    assert not L.sgm_depth_from_both(s, None, f.out_r.ctypes.data, f.out.size, 1000.0, 1001.0, 100.0, 0.0, f.out.ctypes.data)
    L.sgm_destroy(s)


# ---- the host under the sanitizers ------------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_both_family_is_asan_ubsan_clean(tmp_path):
    exe = standin.build(tmp_path, sanitize=True, exe="host_sanitize_driver", extra_sources=standin.SANITIZE_DRIVER)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    out = subprocess.run([exe, "both"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("host_sanitize_driver both ok")
