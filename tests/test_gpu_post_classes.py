"""The map stages behind the winner-take-all on planted maps, kernel by kernel -- needs an MI355X.

The three LR checks (csrc/sgm_sum_wta.hip), the classification and the fill passes (csrc/sgm_fill.hip) run through the device layer
(sgmd_*, csrc/sgm_device.h) on the planted inputs of tests/post_classes.py, the refinement (csrc/sgm_refine.hip) through
sgm_refine_disparity at the line lengths its slab logic turns on.  Expected results are the restatements -- the oracle's two LR
checks, tests/fill_holes_ref.py, tests/refine_ref.py with the library's tables --, tolerance 0, compared as uint32.  After each
comparison the census is recounted from the INPUTS and held to tests/golden/post_classes.json, so that a changed generator cannot
quietly stop planting; tests/test_post_classes_cpu.py shows that each planted branch changes the result when a kernel gets it wrong.

The device-layer calls work on torch buffers, which carry no guard bands: there the three different frames of every input are what
a read across a row end or a frame edge shows in."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import fill_holes_ref as F
import post_classes as PC
from conftest import GOLDEN
from oracle.pyoracle import default_option

pytestmark = pytest.mark.gpu

INF = PC.INF
FILL_NAMES = [f"{s}-{v}" for s, v in PC.FILL_INPUTS]


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={got[first]} want={want[first]}")


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLDEN, "post_classes.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def device():
    import soc_project_stereo_matching_amd as S
    L = S.load_library()
    vp, geo = C.c_void_p, C.POINTER(PC.Geom)
    L.sgmd_lrcheck.argtypes = [C.c_int, vp, geo, vp, vp, C.c_float]
    L.sgmd_lrcheck_right.argtypes = [C.c_int, vp, geo, vp, vp, C.c_float, C.c_int, vp]
    L.sgmd_lrcheck_both.argtypes = [C.c_int, vp, geo, vp, vp, C.c_float, C.c_int, vp, vp]
    L.sgmd_fill_classify.argtypes = [C.c_int, vp, geo, vp, vp, C.c_float, C.c_int, C.c_int, vp]
    L.sgmd_fill_pass.argtypes = [C.c_int, vp, geo, C.c_int, vp, vp, vp, C.c_int]
    L.sgmd_stream_sync.argtypes = [C.c_int, vp]
    for f in (L.sgmd_lrcheck, L.sgmd_lrcheck_right, L.sgmd_lrcheck_both, L.sgmd_fill_classify, L.sgmd_fill_pass, L.sgmd_stream_sync):
        f.restype = C.c_int
    return L


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def marked(shape, dtype=np.float32):
    """an output buffer nobody wrote: a different value in every element, none of them a disparity or a class"""
    n = int(np.prod(shape))
    return (-(1000.0 + np.arange(n) % 9973) if dtype == np.float32 else 200 + np.arange(n) % 50).astype(dtype).reshape(shape)


def launch(fn, g, *args):
    """ordinal 0, the NULL stream, and the call has ended when this returns"""
    import torch
    torch.cuda.synchronize()
    L = device()
    assert fn(0, None, C.byref(g), *[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]) == 0
    assert L.sgmd_stream_sync(0, None) == 0
    torch.cuda.synchronize()


# ---- the three LR checks and the classification -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def device_lr(name):
    """every LR form's output on the device, as numpy"""
    L, p = device(), PC.lr_input(name)
    g = PC.geom(p.W, p.H, PC.B)
    tl, tr = dev(p.dl), dev(p.dr)
    out = {}
    t = dev(p.dl)
    launch(L.sgmd_lrcheck, g, t, tr, C.c_float(p.thres))
    out["left"] = t.cpu().numpy()
    for check in (1, 0):
        t = dev(marked(p.dr.shape))
        launch(L.sgmd_lrcheck_right, g, tr, tl, C.c_float(p.thres), check, t)
        out["right", check] = t.cpu().numpy()
        ol, orr = dev(marked(p.dl.shape)), dev(marked(p.dr.shape))
        launch(L.sgmd_lrcheck_both, g, tl, tr, C.c_float(p.thres), check, ol, orr)
        out["both", check] = (ol.cpu().numpy(), orr.cpu().numpy())
    out["inputs"] = (tl.cpu().numpy(), tr.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def device_classes(name):
    L, p = device(), PC.lr_input(name)
    g = PC.geom(p.W, p.H, PC.B)
    out = {}
    for right in (False, True):
        ref, oth = p.view(right)
        tref, toth = dev(ref), dev(oth)
        for check in (1, 0):
            t = dev(marked(ref.shape, np.uint8))
            launch(L.sgmd_fill_classify, g, tref, toth, C.c_float(p.thres), int(right), check, t)
            out[right, check] = t.cpu().numpy()
    return out


def assert_fixture_counts(name):
    """the census of the INPUTS is the pinned one"""
    got = PC.lr_input(name).counts()
    assert got == golden()["lr"][name]["counts"], f"{name}: the generator plants something else than the fixture says"


@pytest.mark.parametrize("name", list(PC.LR_INPUTS))
def test_lr_checks_on_planted_maps(oracle, name):
    p, got = PC.lr_input(name), device_lr(name)
    want_l, want_r = PC.lr_both(oracle, p.dl, p.dr, p.thres)
    assert_same(got["left"], want_l, f"{name}: sgmd_lrcheck in place")
    assert_same(got["right", 1], want_r, f"{name}: sgmd_lrcheck_right")
    assert_same(got["right", 0], p.dr, f"{name}: sgmd_lrcheck_right without the check")
    assert_same(got["both", 1][0], want_l, f"{name}: sgmd_lrcheck_both, left map")
    assert_same(got["both", 1][1], want_r, f"{name}: sgmd_lrcheck_both, right map")
    assert_same(got["both", 1][0], got["left"], f"{name}: both vs the left kernel")
    assert_same(got["both", 1][1], got["right", 1], f"{name}: both vs the right kernel")
    assert_same(got["both", 0][0], p.dl, f"{name}: sgmd_lrcheck_both without the check, left map")
    assert_same(got["both", 0][1], p.dr, f"{name}: sgmd_lrcheck_both without the check, right map")
    assert_same(got["inputs"][0], p.dl, f"{name}: the left input is only read")
    assert_same(got["inputs"][1], p.dr, f"{name}: the right input is only read")
    assert_fixture_counts(name)


def test_lr_checks_in_a_row_window(oracle):
    L, p = device(), PC.lr_input("96x24")
    r0, r1 = 5, 17
    g = PC.geom(p.W, p.H, PC.B, r0, r1)
    want_l, want_r = PC.lr_both(oracle, p.dl, p.dr, p.thres)
    mark = marked(p.dl.shape)
    inside = np.zeros(p.dl.shape, bool)
    inside[:, r0:r1] = True
    t = dev(np.where(inside, p.dl, mark))
    launch(L.sgmd_lrcheck, g, t, dev(p.dr), C.c_float(p.thres))
    assert_same(t.cpu().numpy(), np.where(inside, want_l, mark), "sgmd_lrcheck rows 5..16")
    t = dev(mark)
    launch(L.sgmd_lrcheck_right, g, dev(p.dr), dev(p.dl), C.c_float(p.thres), 1, t)
    assert_same(t.cpu().numpy(), np.where(inside, want_r, mark), "sgmd_lrcheck_right rows 5..16")


@pytest.mark.parametrize("name", list(PC.LR_INPUTS))
def test_classification_on_planted_maps(name):
    p, got = PC.lr_input(name), device_classes(name)
    for right in (False, True):
        ref, oth = p.view(right)
        assert_same(got[right, 1], PC.classes(ref, oth, p.thres, right), f"{name}: classes, right={right}")
        assert_same(got[right, 0], np.zeros(ref.shape, np.uint8), f"{name}: classes without the check, right={right}")
    assert_fixture_counts(name)


@pytest.mark.parametrize("name", list(PC.LR_INPUTS))
def test_class_nonzero_exactly_where_the_lr_check_leaves_inf(name):
    lr, cls = device_lr(name), device_classes(name)
    for right, maps in ((False, (lr["left"], lr["both", 1][0])), (True, (lr["right", 1], lr["both", 1][1]))):
        for m in maps:
            assert np.array_equal(cls[right, 1] != 0, m == INF), f"{name}: right={right}"


# ---- the fill passes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FILL_NAMES)
def test_single_fill_passes_on_planted_maps(name):
    shape, variant = name.split("-")
    L, p = device(), PC.fill_input(shape, variant)
    g = PC.geom(p.W, p.H, PC.B)
    tc = dev(p.cls)
    for R in PC.FILL_RS:
        before = p.disp
        for ps, want in zip((1, 2, 3), PC.fill_passes(p.disp, p.cls, R)):
            tin, tout = dev(before), dev(marked(before.shape))
            launch(L.sgmd_fill_pass, g, R, tin, tout, tc, ps)
            assert_same(tout.cpu().numpy(), want, f"{name} R={R}: pass {ps}")
            assert_same(tin.cpu().numpy(), before, f"{name} R={R}: pass {ps} only reads its input")
            before = want
        tin, tout = dev(p.disp), dev(marked(p.disp.shape))
        launch(L.sgmd_fill_pass, g, R, tin, tout, None, 3)
        assert_same(tout.cpu().numpy(), F.fill(p.disp, None, R), f"{name} R={R}: pass 3 without classes")
        assert p.counts(R) == golden()["fill"][name]["counts"][str(R)], f"{name} R={R}: the generator plants something else"
    assert_same(tc.cpu().numpy(), p.cls, f"{name}: the classes are only read")


@pytest.mark.parametrize("name", FILL_NAMES)
def test_composed_fill_on_planted_maps(name):
    import soc_project_stereo_matching_amd as S
    shape, variant = name.split("-")
    p = PC.fill_input(shape, variant)
    inst = S.SGMInstance(0, batch=PC.B)
    try:
        for R in PC.FILL_RS:
            assert inst.reset(p.W, p.H, default_option(R)), f"{name} R={R}"
            tc = dev(p.cls)
            for with_classes in (True, False):
                t = dev(p.disp)
                assert inst.fill_holes(t.data_ptr(), tc.data_ptr() if with_classes else None) and inst.synchronize()
                want = F.fill(p.disp, p.cls if with_classes else None, R)
                assert_same(t.cpu().numpy(), want, f"{name} R={R}: sgm_fill_holes, classes={with_classes}")
            assert_same(tc.cpu().numpy(), p.cls, f"{name}: the classes are only read")
            assert p.counts(R) == golden()["fill"][name]["counts"][str(R)]
    finally:
        inst.close()


# ---- the refinement at the line lengths of its slab logic ----------------------------------------------------------------------------

def check_refine(inst, W, H, frames, what):
    from test_gpu_refine import expected
    for disp, conf, guide, all_inf in PC.refine_inputs(W, H, frames):
        for params in PC.REFINE_PARAMS:
            for keep in (False, True):
                assert inst.set_refine(True, *params, keep_invalid=keep)
                td, tc, tg = dev(disp), dev(conf.view(np.int16)), dev(guide)
                assert inst.refine_disparity(td, tc, tg) and inst.synchronize()
                got, want = td.cpu().numpy(), expected(disp, conf, guide, params, keep)
                tag = f"{what} {W}x{H}x{frames} {params} keep={keep} all_inf={all_inf}"
                assert_same(got, want, tag)
                for f in range(frames):                       # the comparison above is about numbers, not about +INF staying +INF
                    assert np.isinf(want[f]).all() if f in all_inf else np.isfinite(want[f]).any(), tag
                assert_same(tg.cpu().numpy(), guide, f"{what}: the guide is only read")


@pytest.mark.parametrize("W,H,frames", PC.REFINE_SHAPES, ids=lambda v: str(v))
def test_refinement_at_the_slab_line_lengths(W, H, frames):
    import soc_project_stereo_matching_amd as S
    inst = S.SGMInstance(0, batch=frames)
    try:
        assert inst.reset(W, H, default_option(16))
        check_refine(inst, W, H, frames, "refine")
    finally:
        inst.close()


# ---- the public entry points under guard bands ----------------------------------------------------------------------------------------

def test_under_guard_bands(monkeypatch):
    """the debug allocation mode around the ping-pong map of the fill and the U, V, Q maps of the refinement, at 33 x 7 and 65 x 1"""
    import torch
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(1 << 20))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    inst = S.SGMInstance(0, batch=PC.B)
    try:
        for (W, H) in ((33, 7), (65, 1)):
            rng = np.random.default_rng(W * H)
            disp = (rng.integers(-8, 64, (PC.B, H, W)) / np.float32(4)).astype(np.float32)
            disp[rng.random(disp.shape) < 0.6] = INF
            disp[1, :, W // 2:] = INF
            cls = rng.integers(0, 3, disp.shape).astype(np.uint8)
            for R in (7, 64):
                assert inst.reset(W, H, default_option(R))
                tc = dev(cls)
                for c in (cls, None):
                    t = dev(disp)
                    assert inst.fill_holes(t.data_ptr(), tc.data_ptr() if c is not None else None) and inst.synchronize()
                    assert_same(t.cpu().numpy(), F.fill(disp, c, R), f"guarded fill {W}x{H} R={R} classes={c is not None}")
            check_refine(inst, W, H, PC.B, "guarded refine")
        torch.cuda.synchronize()
        bad, live, size = S.debug_guard_check()
        assert bad == 0 and live > 0 and size > 0
    finally:
        inst.close()
    assert S.debug_guard_check() == (0, 0, 0)
