"""The planted inputs of tests/post_classes.py on the CPU: they reproduce the digests and counts of tests/golden/post_classes.json
(made by tests/golden/make_golden_post_classes.py from the restatements alone), the census equals the restatements on every input
and in both views, every branch is taken by at least 20 pixels on the quota inputs, and every listed mistake of a kernel -- a
one-line mutant of the contract's steps below -- changes the result on at least one planted input, so that the comparison of
tests/test_gpu_post_classes.py can fail for it.

Quotas.  LR checks and classes: every branch of post_classes.LR_BRANCHES, per view, on 96x24 (thres 1.0 and 0.1f) and 257x5, counted
over the three frames.  Excused: none in either view -- a negative disparity walks the left view off the right edge, and a
disparity of k + 0.5 -+ 2^-24 makes the float32 sum part from the exact one at any column.  Fill: every k0 .. k8 and every
named mask per pass, over the inputs of 61x47 and 17x5 and every R together.  Excused: copied_other_class in pass 3, which takes
every +INF pixel whatever its class."""
import functools
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import fill_holes_ref as F
import post_classes as PC
from conftest import GOLDEN, ROOT
from oracle.pyoracle import sha

INF, F32, F64 = PC.INF, np.float32, np.float64
FILL_NAMES = [f"{s}-{v}" for s, v in PC.FILL_INPUTS]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLDEN, "post_classes.json")) as f:
        return json.load(f)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

def test_generator_reproduces_the_fixture_byte_for_byte():
    spec = importlib.util.spec_from_file_location("make_golden_post_classes", os.path.join(GOLDEN, "make_golden_post_classes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "post_classes.json")) as f:
        text = f.read()
    assert json.dumps(mod.document(), indent=1) + "\n" == text
    doc = golden()
    assert sorted(doc["lr"]) == sorted(PC.LR_INPUTS) and sorted(doc["fill"]) == sorted(FILL_NAMES) and doc["floor"] == PC.FLOOR == 20


@pytest.mark.parametrize("name", list(PC.LR_INPUTS))
def test_lr_inputs_and_outputs_reproduce_the_digests(oracle, name):
    p, want = PC.lr_input(name), golden()["lr"][name]
    assert want["seed"] == p.seed and want["shape"] == [p.W, p.H, 3] and want["options"]["lrcheck_thres"] == p.thres
    assert p.dl.shape == p.dr.shape == (3, p.H, p.W)
    assert sha(p.dl) == want["sha256_inputs"]["disp_l"] and sha(p.dr) == want["sha256_inputs"]["disp_r"]
    if p.W * p.H > 1:
        assert not same(p.dl[0], p.dl[1]) and not same(p.dl[1], p.dl[2]) and not same(p.dr[0], p.dr[1])   # three different frames
    left, right = PC.lr_both(oracle, p.dl, p.dr, p.thres)
    out = want["sha256_outputs"]
    assert sha(left) == out["lr_left"] == out["lr_both_left"] and sha(right) == out["lr_right"] == out["lr_both_right"]
    assert sha(PC.classes(p.dl, p.dr, p.thres, False)) == out["classes_left"]
    assert sha(PC.classes(p.dr, p.dl, p.thres, True)) == out["classes_right"]


@pytest.mark.parametrize("name", FILL_NAMES)
def test_fill_inputs_and_outputs_reproduce_the_digests(name):
    shape, variant = name.split("-")
    p, want = PC.fill_input(shape, variant), golden()["fill"][name]
    assert want["seed"] == p.seed and want["shape"] == [p.W, p.H, 3] and want["options"]["R"] == list(PC.FILL_RS)
    assert sha(p.disp) == want["sha256_inputs"]["disp"] and sha(p.cls) == want["sha256_inputs"]["classes"]
    for R in PC.FILL_RS:
        out = want["sha256_outputs"][str(R)]
        p1, p2, p3 = PC.fill_passes(p.disp, p.cls, R)
        assert [sha(p1), sha(p2), sha(p3)] == [out["pass1"], out["pass2"], out["pass3"]]
        assert sha(F.fill(p.disp, p.cls, R)) == out["fill"] == out["pass3"]
        assert sha(F.fill(p.disp, None, R)) == out["fill_without_classes"]


# ---- the census equals the restatements -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", PC.VIEWS)
@pytest.mark.parametrize("name", list(PC.LR_INPUTS))
def test_lr_census_equals_the_restatements(oracle, name, view):
    p, right = PC.lr_input(name), view == "right"
    ref, oth = p.view(right)
    m = p.census(right)
    cls = PC.classes(ref, oth, p.thres, right)
    lr = PC.lr_right(oracle, ref, oth, p.thres) if right else PC.lr_left(oracle, ref, oth, p.thres)
    assert np.array_equal(cls == 1, m["back_inf"] | m["back_gt"])
    assert np.array_equal(cls != 0, m["inf"] | m["out_lo"] | m["out_hi"] | m["fail"])
    assert np.array_equal(lr == INF, cls != 0)                         # "Class != 0 exactly where the LR check leaves +INF"
    assert same(lr[cls == 0], ref[cls == 0])
    # the masks partition what they say they partition
    fin = ~m["inf"]
    parts = (m["out_lo"], m["out_hi"], m["other_inf"], m["pass"], m["fail"])
    assert np.array_equal(sum(q.astype(int) for q in parts), fin.astype(int))
    backs = [m[n] for n in ("back_lo", "back_hi", "back_inf", "back_eq", "back_gt", "back_lt")]
    assert np.array_equal(sum(q.astype(int) for q in backs), m["fail"].astype(int))
    assert not (m["eq_thres"] & ~m["pass"]).any() and not (m["ulp_over"] & ~m["fail"]).any()
    assert not (m["trunc0"] & (m["out_lo"] | m["out_hi"])).any()
    assert PC.counts(m) == golden()["lr"][name]["counts"][view]


@pytest.mark.parametrize("name", FILL_NAMES)
def test_fill_census_equals_the_restatements(name):
    shape, variant = name.split("-")
    p = PC.fill_input(shape, variant)
    for R in PC.FILL_RS:
        masks, outs = PC.fill_census(p.disp, p.cls, R)
        for k, want in enumerate(PC.fill_passes(p.disp, p.cls, R)):
            assert same(outs[k + 1], want), f"{name} R={R}: pass {k + 1}"
        assert same(outs[3], F.fill(p.disp, p.cls, R))
        m3, o3 = PC.fill_census(p.disp, None, R)
        assert same(o3[3], F.fill(p.disp, None, R)) and list(m3) == [3]
        before = {1: p.disp, 2: outs[1], 3: outs[2]}
        for ps in (1, 2, 3):
            m = masks[ps]
            targets = (before[ps] == INF) & (True if ps == 3 else p.cls == ps)
            assert np.array_equal(sum(m[n].astype(int) for n in PC.FILL_K), targets.astype(int))
            assert np.array_equal(outs[ps] == INF, (before[ps] == INF) & ~(targets & ~m["k0"]))    # filled: exactly the targets with a candidate
            assert not (m["k0"] & (m["hit_at_R"] | m["dup"])).any() and not (m["copied_other_class"] & targets).any()
        assert {str(ps): PC.counts(m) for ps, m in masks.items()} == golden()["fill"][name]["counts"][str(R)]


def test_census_on_a_hand_made_row():
    """W = 8, left view, thres 1: one pixel per column decision"""
    ref = np.array([[1.25, 0.75, 2.5, -5.5, INF, 5.0 + 2.0 ** -21, 1.5, 0.5 + 2.0 ** -24]], F32)
    #  x = 0: 0 - 1.25 + .5 = -0.75 -> column 0 (trunc0);  x = 1: 0.25 + .5 -> 0;  x = 2: -0.5 (half) + .5 = 0 -> 0
    #  x = 3: 8.5 (half) + .5 = 9 -> out_hi;  x = 5: -2^-21 + .5 -> 0;  x = 6: 4.5 (half) -> 5;  x = 7: float 6.5 -> 7, exact 6
    oth = np.array([[1.25, 0, 0, 0, 0, INF, 0, 0.5]], F32)
    m = PC.census(ref, oth, 1.0, False)
    got = {n: np.flatnonzero(q[0]).tolist() for n, q in m.items()}
    assert got["inf"] == [4] and got["out_hi"] == [3] and got["out_lo"] == [] and got["trunc0"] == [0]
    assert got["half"] == [2, 3, 6, 7] and got["f32_sum"] == [7] and got["other_inf"] == [6]    # (7: the FLOAT sum is 6.5)
    # x = 0, 1, 2, 5 read oth[0] = 1.25: |d - o| = 0, 0.5, 1.25, 3.75 + 2^-21;  x = 7 reads oth[7]: 2^-24
    assert got["pass"] == [0, 1, 7] and got["fail"] == [2, 5] and got["eq_thres"] == [] and got["ulp_over"] == []
    # x = 2 and 5 point back at 0 + 1.25 + .5 -> column 1: ref[1] = 0.75 < 2.5 and < 5
    assert got["back_lt"] == [2, 5]
    cls = F.classify(ref, oth, 1.0)
    assert cls.tolist() == [[0, 0, 2, 2, 2, 2, 0, 0]]
    # the thresholds: |0.5 - 1.5| == 1 kept, one ulp of 1 more rejected; the right view reads column x + d (0.5 + .5 -> 1, 2)
    ref = np.array([[0.5, 0.5, INF, INF]], F32)
    oth = np.array([[INF, 1.5, np.nextafter(F32(1.5), INF), INF]], F32)
    m = PC.census(ref, oth, 1.0, True)
    assert np.flatnonzero(m["eq_thres"][0]).tolist() == [0] and np.flatnonzero(m["ulp_over"][0]).tolist() == [1]
    assert np.flatnonzero(m["back_eq"][0]).tolist() == [1]            # column 2 - 1.5000001 + .5 -> 0: ref[0] == 0.5
    assert F.classify(ref, oth, 1.0, right=True).tolist() == [[0, 2, 2, 2]]


# ---- quotas -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", PC.VIEWS)
@pytest.mark.parametrize("name", PC.QUOTA_INPUTS)
def test_lr_quotas(name, view):
    got = PC.lr_input(name).counts()[view]
    assert got == golden()["lr"][name]["counts"][view]
    for n in PC.LR_BRANCHES:
        assert got[n] >= PC.FLOOR, f"{name}: {view} view: branch {n}: {got[n]} pixels"


def test_the_wide_input_parts_the_float32_sum_from_the_exact_one():
    got = PC.lr_input("65535x2").counts()
    for view in PC.VIEWS:
        assert got[view]["f32_sum"] >= 20000, got[view]["f32_sum"]


def test_fill_quotas():
    total = {str(ps): dict.fromkeys(PC.FILL_MASKS, 0) for ps in (1, 2, 3)}
    for shape in PC.FILL_QUOTA_SHAPES:
        for variant in PC.FILL_VARIANTS:
            want = golden()["fill"][f"{shape}-{variant}"]["counts"]
            for R in PC.FILL_RS:
                got = PC.fill_input(shape, variant).counts(R)
                assert got == want[str(R)]
                for ps, c in got.items():
                    for n, v in c.items():
                        total[ps][n] += v
    for ps in (1, 2, 3):
        for n in PC.FILL_MASKS:
            if n in PC.FILL_EXCUSED[ps]:
                assert total[str(ps)][n] == 0
            else:
                assert total[str(ps)][n] >= PC.FLOOR, f"pass {ps}: {n}: {total[str(ps)][n]} targets"


# ---- the inputs discriminate: one-line mutants of the contract's steps -----------------------------------------------------------

STEPS = {
    "sum": lambda x, sd: x.astype(F32) + sd,                                             # float32
    "round": lambda s: np.trunc(s.astype(F64) + 0.5),                                    # double add, truncation toward zero
    "over": lambda d, o, thres: np.abs((d - o).astype(F64)) > F64(F32(thres)),           # float32 difference, strict compare in double
    "other_inf_rejects": False,
    "nearer": lambda r, d: r > d,                                                        # +INF counts as larger
    "back_in": lambda xb, W: (xb >= 0) & (xb < W),
    "back_sign": lambda sgn: -sgn,
}

LR_MUTANTS = {
    "floor instead of truncation": dict(round=lambda s: np.floor(s.astype(F64) + 0.5)),
    "the sum in double": dict(sum=lambda x, sd: x.astype(F64) + sd.astype(F64)),
    "round-half-even": dict(round=lambda s: np.rint(s.astype(F64))),
    ">= for the threshold": dict(over=lambda d, o, thres: np.abs((d - o).astype(F64)) >= F64(F32(thres))),
    "the compare in float32 against thres as double": dict(over=lambda d, o, thres: np.abs(d - o).astype(F64) > F64(thres)),
    "an other_inf pixel rejected": dict(other_inf_rejects=True),
    "ref[xb] >= d": dict(nearer=lambda r, d: r >= d),
    "ref[xb] == INF counted as class 2": dict(nearer=lambda r, d: (r != INF) & (r > d)),
    "xb clamped instead of bounds-checked": dict(back_in=lambda xb, W: np.ones(xb.shape, bool)),
    "the right view's signs swapped in the back projection only": dict(back_sign=lambda sgn: F32(1)),
}


def contract(ref, oth, thres, right, **change):
    """(LR output, classes) of a batch by the contract's steps, any of them replaced"""
    st = dict(STEPS, **change)
    W = ref.shape[-1]
    x = np.broadcast_to(np.arange(W), ref.shape)
    sgn = F32(1) if right else F32(-1)
    fin = ref != INF
    d = np.where(fin, ref, F32(0))
    col = st["round"](st["sum"](x, sgn * d)).astype(np.int64)
    inb = fin & (col >= 0) & (col < W)
    o = np.take_along_axis(oth, np.clip(col, 0, W - 1), axis=-1)
    seen = inb & (o != INF)
    o0 = np.where(seen, o, F32(0))
    rejected = seen & st["over"](d, o0, thres)
    if st["other_inf_rejects"]:
        rejected |= inb & (o == INF)
    xb = st["round"](st["sum"](col, st["back_sign"](sgn) * o0)).astype(np.int64)
    r = np.take_along_axis(ref, np.clip(xb, 0, W - 1), axis=-1)
    cls = np.where(~inb | rejected, 2, 0).astype(np.uint8)
    cls[rejected & st["back_in"](xb, W) & st["nearer"](r, d)] = 1
    return np.where(cls != 0, INF, ref), cls


def lr_restated(oracle, p, right):
    ref, oth = p.view(right)
    lr = PC.lr_right(oracle, ref, oth, p.thres) if right else PC.lr_left(oracle, ref, oth, p.thres)
    return lr, PC.classes(ref, oth, p.thres, right)


def test_the_unchanged_steps_are_the_contract(oracle):
    for name in PC.LR_INPUTS:
        p = PC.lr_input(name)
        for right in (False, True):
            lr, cls = contract(*p.view(right), p.thres, right)
            want_lr, want_cls = lr_restated(oracle, p, right)
            assert same(lr, want_lr) and same(cls, want_cls), (name, right)


@pytest.mark.parametrize("mutant", list(LR_MUTANTS))
def test_lr_mutants_are_caught(oracle, mutant):
    caught = []
    for name in PC.LR_INPUTS:
        p = PC.lr_input(name)
        for right in (False, True):
            lr, cls = contract(*p.view(right), p.thres, right, **LR_MUTANTS[mutant])
            want_lr, want_cls = lr_restated(oracle, p, right)
            if not (same(lr, want_lr) and same(cls, want_cls)):
                caught.append((name, "right" if right else "left", int((bits(lr) != bits(want_lr)).sum()), int((cls != want_cls).sum())))
    assert caught, f"no planted input tells '{mutant}' from the contract"


def loop_fill(disp, cls, R, pick1=lambda k: 1 if k >= 2 else 0, pick23=lambda k: k // 2, reach=lambda R: R, frames=True, jacobi=True):
    """the three passes on a batch in plain loops, any step replaced"""
    m = np.array(disp, F32, copy=True)
    if not frames:                                                    # the batch as one tall frame
        m, cls = m.reshape(1, -1, m.shape[-1]), cls.reshape(1, -1, cls.shape[-1])
    h, w = m.shape[-2:]
    for p in (1, 2, 3):
        for f in range(m.shape[0]):
            src = m[f].copy() if jacobi else m[f]
            for y in range(h):
                for x in range(w):
                    if src[y, x] != INF or (p != 3 and cls[f, y, x] != p):
                        continue
                    cand = []
                    for dx, dy in F.RAYS:
                        for step in range(1, reach(R) + 1):
                            yy, xx = y + dy * step, x + dx * step
                            if not (0 <= yy < h and 0 <= xx < w):
                                break
                            if src[yy, xx] != INF:
                                cand.append(src[yy, xx])
                                break
                    if cand:
                        cand.sort()
                        m[f, y, x] = cand[pick1(len(cand)) if p == 1 else pick23(len(cand))]
    return m.reshape(np.shape(disp))


FILL_MUTANTS = {
    "s[(k-1)/2]": dict(pick23=lambda k: (k - 1) // 2),
    "pass 1 taking s[0] always": dict(pick1=lambda k: 0),
    "walking R - 1 steps": dict(reach=lambda R: R - 1),
    "walking R + 1 steps": dict(reach=lambda R: R + 1),
    "ignoring the frame edge between batch frames": dict(frames=False),
    "Gauss-Seidel instead of Jacobi": dict(jacobi=False),
}
SMALL_FILL = [(s, v) for s, v in PC.FILL_INPUTS if s != "61x47"]       # plain loops: the small shapes carry every case but the counts


def test_the_unchanged_loops_are_the_fill():
    for s, v in SMALL_FILL:
        p = PC.fill_input(s, v)
        for R in PC.FILL_RS:
            assert same(loop_fill(p.disp, p.cls, R), F.fill(p.disp, p.cls, R)), (s, v, R)


@pytest.mark.parametrize("mutant", list(FILL_MUTANTS))
def test_fill_mutants_are_caught(mutant):
    caught = []
    for s, v in SMALL_FILL:
        p = PC.fill_input(s, v)
        for R in PC.FILL_RS:
            got, want = loop_fill(p.disp, p.cls, R, **FILL_MUTANTS[mutant]), F.fill(p.disp, p.cls, R)
            if not same(got, want):
                caught.append((p.name, R, int((bits(got) != bits(want)).sum())))
    assert caught, f"no planted input tells '{mutant}' from the contract"
    if mutant == "ignoring the frame edge between batch frames":
        assert any(n.endswith("edges") for n, _, _ in caught)          # the lone corner next to a full frame sees it


# ---- the refinement inputs say something -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,frames", PC.REFINE_SHAPES, ids=lambda v: str(v))
def test_refinement_inputs_are_not_vacuous(W, H, frames):
    """every frame that is not the all-INF one has weight: its expected output (numpy's tables here; the device test takes the
    library's) has finite samples, and where a line has a neighbour to smooth with they are not a copy of the input"""
    import refine_ref as R
    inputs = PC.refine_inputs(W, H, frames)
    assert any(all_inf for *_, all_inf in inputs)                      # one frame or one input all +INF
    for disp, conf, guide, all_inf in inputs:
        for lam, sigma, T in PC.REFINE_PARAMS:
            for keep in (False, True):
                want = R.refine(disp, conf, guide, R.tables(lam, sigma, T), keep)
                for f in range(frames):
                    if f in all_inf:
                        assert np.isinf(disp[f]).all() and np.isinf(want[f]).all()
                        continue
                    fin = np.isfinite(want[f])
                    assert fin.any() and np.isfinite(disp[f]).any() and (conf[f][np.isfinite(disp[f])] > 0).any(), (f, lam, keep)
                    if W * H > 1:
                        assert (bits(want[f])[fin] != bits(disp[f])[fin]).any(), (f, lam, keep)
                    if not keep and W * H > 1 and np.isinf(disp[f]).any():
                        assert (fin & np.isinf(disp[f])).any(), (f, lam, keep)       # a hole took a value from its line


# ---- the ctypes mirror of sgmd_geom ------------------------------------------------------------------------------------------------

def test_geom_mirror_follows_the_header():
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_device.h")) as f:
        text = f.read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*sgmd_geom;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, names = decl.split(None, 1)
            assert kind == "int", decl
            fields += [n.strip() for n in names.split(",")]
    assert tuple(fields) == PC.GEOM_FIELDS == tuple(n for n, _ in PC.Geom._fields_)
    assert all(t is PC.C.c_int for _, t in PC.Geom._fields_) and PC.C.sizeof(PC.Geom) == 4 * len(fields)
    g = PC.geom(96, 24, 3, 5, 17)
    assert (g.W, g.H, g.B, g.row_begin, g.row_end) == (96, 24, 3, 5, 17) and PC.geom(7, 9, 1).row_end == 9
