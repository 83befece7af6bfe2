"""The temporal filter (extension; the contract is in include/sgm_mi355x.h, sgm_temporal_spec) without a GPU: the numpy restatement
tests/temporal_ref.py against one-pixel sequences worked by hand, the C stand-in tests/stub_temporal.c against the restatement on the
kernel tests' random inputs (two independent restatements of the contract), header / library / Python agreement, the C host's logic
on the stand-in device -- validation, where the launch sits, the history's lifetime, refusals -- and a sanitizer run of a
stand-alone driver.  Tolerance 0 everywhere."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import standin
import temporal_cases as TC
import temporal_ref as TR
from conftest import ROOT

STUB_TEMPORAL = os.path.join(ROOT, "tests", "stub_temporal.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement against sequences worked by hand -------------------------------------------------------------------------

def walk(spec, xs, hv=INF, hb=0, conf=None):
    """one pixel through the inputs xs: [(out, hv, hb, class)] per step"""
    hv, hb = np.array([hv], np.float32), np.array([hb], np.uint8)
    rows = []
    for t, x in enumerate(xs):
        out, hv, hb, cls = TR.step(spec, hv, hb, np.array([x], np.float32), None if conf is None else np.array([conf[t]], np.uint16))
        rows.append((out[0], hv[0], int(hb[0]), TR.CLASSES[int(cls[0])]))
    return rows


def test_every_class_and_the_forget_rule_by_hand():
    spec = TR.Spec(0.5, 1.0, 3, 2)
    rows = walk(spec, [10, 11, 12, INF, NAN, -INF, INF, INF, INF, INF, INF, 5])
    f = np.float32
    want = [(f(10), f(10), 0b1, "first"),
            (f(10.5), f(10.5), 0b11, "smoothed"),            # |11 - 10| == delta exactly: inside the gate; 0.5 * 11 + 0.5 * 10
            (f(12), f(12), 0b111, "replaced"),               # |12 - 10.5| = 1.5 > 1
            (f(12), f(12), 0b1110, "held"),                  # three of the last three inputs valid
            (f(12), f(12), 0b11100, "held"),                 # two of three: k = 2 still holds
            (INF, f(12), 0b111000, "invalid"),               # one of three: refused; the history keeps its value
            (INF, f(12), 0b1110000, "invalid"),
            (INF, f(12), 0b11100000, "invalid"),
            (INF, f(12), 0b11000000, "invalid"),
            (INF, f(12), 0b10000000, "invalid"),
            (INF, INF, 0, "invalid"),                        # the eighth invalid input in a row: forgotten
            (f(5), f(5), 1, "first")]
    assert len(rows) == len(want)
    for t, (got, exp) in enumerate(zip(rows, want)):
        assert same_bits(np.array(got[:2], np.float32), np.array(exp[:2], np.float32)) and got[2:] == exp[2:], (t, got, exp)


def test_a_held_value_does_not_keep_itself_alive():
    """the validity bits record inputs: with k = 1 of n = 2 a hole is bridged for two frames and no longer"""
    rows = walk(TR.Spec(0.5, 1.0, 2, 1), [7, NAN, NAN, NAN, NAN])
    assert [r[3] for r in rows] == ["first", "held", "held", "invalid", "invalid"]
    assert [r[0] for r in rows[1:3]] == [7, 7] and np.isposinf(rows[3][0]) and rows[4][1] == 7


def test_alpha_one_delta_zero_and_the_rounding_of_the_blend():
    f = np.float32
    assert walk(TR.Spec(1.0, 1.0, 0, 1), [10.5], hv=10, hb=1)[0][:2] == (f(10.5), f(10.5))          # 1 * x + 0 * hv
    nxt = np.nextafter(f(10), f(20), dtype=np.float32)
    assert walk(TR.Spec(0.25, 0.0, 0, 1), [10], hv=10, hb=1)[0][3] == "smoothed"                   # |x - hv| == 0 == delta
    assert walk(TR.Spec(0.25, 0.0, 0, 1), [nxt], hv=10, hb=1)[0][3] == "replaced"
    # 0 hold window: never held, whatever the bits say
    assert walk(TR.Spec(0.25, 0.0, 0, 1), [NAN], hv=10, hb=0xFF)[0][3] == "invalid"
    # a = f32(0.4), b = f32(1) - a, two products and one sum, each rounded to float32
    a = f(0.4)
    b = f(1.0) - a
    x, hv = f(20.3), f(19.9)
    assert walk(TR.Spec(0.4, 1.0, 0, 1), [x], hv=hv, hb=1)[0][0] == f(f(a * x) + f(b * hv))
    # subnormals are kept: half of the smallest normal plus half of it
    tiny = f(1.1754944e-38)
    assert walk(TR.Spec(0.5, 1.0, 0, 1), [tiny], hv=0.0, hb=1)[0][0] == f(tiny * f(0.5)) != 0


def test_confidence_gate_and_caller_made_state():
    spec = TR.Spec(0.5, 1.0, 2, 1, 100)
    rows = walk(spec, [8, 8, 8], conf=[99, 100, 0])
    assert [r[3] for r in rows] == ["invalid", "first", "held"]
    assert [r[3] for r in walk(spec._replace(min_conf=0), [8, 8, 8], conf=[99, 100, 0])] == ["first", "smoothed", "smoothed"]
    # arbitrary caller-made history: NaN and -INF are "not finite"; a held value is the history's own bits
    assert walk(TR.Spec(0.5, 1.0, 2, 1), [4], hv=NAN, hb=3)[0][3] == "first"
    assert walk(TR.Spec(0.5, 1.0, 2, 1), [NAN], hv=-INF, hb=3)[0][3] == "invalid"
    assert walk(TR.Spec(0.5, 1.0, 2, 1), [NAN], hv=-INF, hb=3)[0][1] == -INF                     # hb' != 0: the history stays as it is


def test_run_orders_the_steps_and_counts_exactly():
    spec = TR.Spec(0.4, 0.5, 3, 2, TC.MIN_CONF)
    maps, conf, hv, hb = TC.inputs((777, 2, 3, False), spec)
    out, hv1, hb1, stats = TR.run(spec, maps, conf, hv, hb)
    assert stats.shape == (6, 5) and np.all(stats.sum(axis=1) == 777)
    # three steps in one call are three calls of one step
    h, b = hv, hb
    for t in range(3):
        o, h, b, st = TR.run(spec, maps[:, t:t + 1], conf[:, t:t + 1], h, b)
        assert same_bits(o[:, 0], out[:, t]) and np.array_equal(st[:, :], stats[[t, 3 + t]])
    assert same_bits(h, hv1) and same_bits(b, hb1)


@pytest.mark.parametrize("k", range(len(TC.PARAMS)))
def test_the_kernel_cases_reach_every_class_the_parameters_admit(k):
    """per parameter set, every class the parameters admit occurs at least 100 times over the shapes with >= 4096 pixels"""
    total = dict.fromkeys(TR.CLASSES + ("forgets",), 0)
    for shape in TC.SHAPES:
        if shape[0] < 4096:
            continue
        for name, n in TC.histogram(TC.PARAMS[k], *TC.inputs(shape, TC.PARAMS[k])).items():
            total[name] += n
    for name in TC.ADMITS[k]:
        assert total[name] >= 100, (TC.PARAMS[k], total)
    if "held" not in TC.ADMITS[k]:
        assert total["held"] == 0


@pytest.mark.parametrize("name", TC.PAIRS[:6])
def test_the_match_sequences_reach_every_class_on_every_tiny_pair(oracle, golden_cases, name):
    """six noisy frames of a golden pair, the fourth almost entirely invalid, parameters (0.4, 0.125, 3, 2): every class at least
    ten times (with delta 1.0 several of the pairs have no replaced pixel at all, which is why the GPU tests use 0.125)"""
    from conftest import case_inputs, option_from_dict
    case = golden_cases[name]
    opt = option_from_dict(case["option"])
    finals = [oracle.run(l, r, opt)["final"] for l, r in TC.frames_of(*case_inputs(case, oracle))]
    total = sum(row[3] for row in TC.filtered(TC.MATCH_SPEC, finals))
    assert np.all(total >= 10), (name, dict(zip(TR.CLASSES, total.tolist())))
    assert np.isfinite(finals[TC.BLANK]).sum() < finals[0].size // 20


# ---- header, library, Python ------------------------------------------------------------------------------------------------

NEW = ("sgm_temporal_filter", "sgm_temporal_clear", "sgm_set_temporal", "sgm_temporal_restart", "sgm_temporal_stats", "SGM_SetTemporal",
       "SGM_TemporalRestart", "SGM_TemporalStats")


def test_header_library_and_python_agree():
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    lib = S.load_library()
    declared = _declared_functions()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    for name in ("sgmd_temporal", "sgmd_temporal_clear"):
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    assert C.sizeof(S.SGMTemporalSpec) == 28
    order = ["alpha", "delta", "hold_window", "hold_count", "sequence", "min_conf", "stats"]
    assert [f[0] for f in S.SGMTemporalSpec._fields_] == order
    for k, name in enumerate(order):
        assert getattr(S.SGMTemporalSpec, name).offset == 4 * k and getattr(S.SGMTemporalSpec, name).size == 4, name
    body = re.search(r"typedef struct \{([^}]*)\} sgm_temporal_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [decl.split()[-1] for decl in body.split(";") if decl.strip()] == order
    for m in ("set_temporal", "temporal_restart", "temporal_stats", "temporal_filter", "temporal_clear", "read_temporal"):
        assert callable(getattr(S.SGMInstance, m, None)), m
    for m in ("set_temporal", "temporal_restart", "temporal_stats", "read_temporal"):
        assert callable(getattr(S.SGM, m, None)), m
    assert S.TEMPORAL_CLASSES == TR.CLASSES
    sp = S.temporal_spec()
    assert (sp.hold_window, sp.sequence, sp.min_conf, sp.stats) == (0, 0, 0, 0)
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "Makefile")) as fh:
        assert re.search(r"^HIP_UNITS\s*:=.*\bsgm_temporal\b", fh.read(), re.M)


def test_kernel_resources_keep_eight_waves_per_simd(tmp_path):
    """the compile-time gate: 0 bytes of scratch in every instantiation and at most 64 VGPRs (profiles/temporal_resources.txt)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", fh.read(), re.M | re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sgm_temporal.hip"), "-o",
                          str(tmp_path / "sgm_temporal.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(vgprs) == len(scratch) == 10 and sum("sgm_temporal_k" in n for n in names) == 8, names
    assert max(vgprs) <= 64 and not any(scratch), list(zip(names, vgprs, scratch))
    with open(os.path.join(ROOT, "profiles", "temporal_resources.txt")) as fh:
        table = fh.read()
    assert [int(row.split()[-8]) for row in table.splitlines() if row.startswith("sgm_") and " / " in row] == vgprs        # the committed table is this build's


# ---- the C stand-in against the restatement ------------------------------------------------------------------------------------

class DeviceParams(C.Structure):                                 # sgmd_temporal_params of csrc/sgm_device.h, as the stand-in logs it
    _fields_ = [("a", C.c_float), ("b", C.c_float), ("delta", C.c_float), ("n", _i), ("k", _i), ("min_conf", C.c_uint)]


def _sign(L):
    for name, (res, args) in {"sgm_temporal_filter": (_b, [_p, _p, _z, _z, _z] + [_p] * 5), "sgm_temporal_clear": (_b, [_p, _z, _z, _p, _p]),
                              "sgm_set_temporal": (_b, [_p, _p]), "sgm_temporal_restart": (_b, [_p]), "sgm_temporal_stats": (_i, [_p, _p, _i]),
                              "SGM_SetTemporal": (_b, [_p]), "SGM_TemporalRestart": (_b, []), "SGM_TemporalStats": (_i, [_p, _i]),
                              "SGM_Initialize": (_b, [C.c_uint16, C.c_uint16, _p]), "SGM_Reset": (_b, [C.c_uint16, C.c_uint16, _p]),
                              "SGM_Match": (_b, [_p] * 3), "SGM_Shutdown": (None, []), "sgm_stream": (_p, [_p]),
                              "stub_temporal_clear_log": (None, []), "stub_temporal_count": (_i, []), "stub_temporal_kind": (_i, [_i]),
                              "stub_temporal_geometry": (_z, [_i, _i]), "stub_temporal_ptr": (_p, [_i, _i]),
                              "stub_temporal_params": (C.POINTER(DeviceParams), [_i]), "stub_temporal_fail_at": (None, [_i]),
                              "stub_temporal_cap": (None, [_z]), "stub_temporal_at": (_i, [_i]), "stub_temporal_stream": (_p, [_i]),
                              "stub_fail_alloc_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("temporalstub"), extra_sources=[STUB_TEMPORAL], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("temporalstub_without"), flags=("-ffp-contract=off",)))


def c_spec(spec, sequence=0, stats=0):
    import soc_project_stereo_matching_amd as S
    return S.SGMTemporalSpec(spec.alpha, spec.delta, spec.n, spec.k, sequence, spec.min_conf, stats)


def offset_copy(a, elements):
    """a copy of `a` that starts `elements` elements into a 64-byte aligned buffer: its address is aligned to the element and no more"""
    raw = np.zeros(a.size + elements + 64, a.dtype)
    skip = (-raw.ctypes.data % 64) // a.itemsize + elements
    view = raw[skip:skip + a.size].reshape(a.shape)
    view[...] = a
    return view


def filter_on(L, s, spec, maps, conf, hv, hb, stats=True, misaligned=False):
    """sgm_temporal_filter on copies of the inputs -> (maps, hv, hb, stats or None) as the call left them"""
    maps, hv, hb = (offset_copy(maps, 1) if misaligned else maps.copy()), hv.copy(), hb.copy()
    conf = None if conf is None else (offset_copy(conf, 1) if misaligned else conf.copy())
    streams, steps, pixels = maps.shape
    st = np.full((streams * steps, 5), 0xA5A5A5A5, np.uint32) if stats else None
    sp = c_spec(spec)
    assert L.sgm_temporal_filter(s, C.byref(sp), streams, steps, pixels, maps.ctypes.data, None if conf is None else conf.ctypes.data,
                                 hv.ctypes.data, hb.ctypes.data, None if st is None else st.ctypes.data)
    return maps, hv, hb, st


@pytest.mark.parametrize("k", range(len(TC.PARAMS)))
@pytest.mark.parametrize("shape", [s for s in TC.SHAPES if s[0] <= 60000], ids=TC.shape_id)
def test_stand_in_equals_the_restatement_bit_for_bit(host, shape, k):
    spec = TC.PARAMS[k]
    maps, conf, hv, hb = TC.inputs(shape, spec)
    host.stub_temporal_cap(1 << 30)
    s = host.sgm_create(0)
    try:
        for with_conf in (True, False):
            want = TR.run(spec, maps, conf if with_conf else None, hv, hb)
            for with_stats in (True, False):
                got = filter_on(host, s, spec, maps, conf if with_conf else None, hv, hb, with_stats, shape[3])
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2]), (with_conf, with_stats)
                if with_stats:
                    assert np.array_equal(got[3], want[3])
    finally:
        host.stub_temporal_cap(1 << 20)
        host.sgm_destroy(s)


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

W, H = 48, 20
GOOD = TR.Spec(0.4, 0.125, 3, 2)


def option():
    import soc_project_stereo_matching_amd as S
    return S.default_option(16)


def make(L, spec=GOOD, w=W, h=H, batch=1, sequence=0, stats=1):
    s = L.sgm_create(0)
    assert s
    opt = option()
    sp = c_spec(spec, sequence, stats)
    assert L.sgm_set_batch(s, batch) and L.sgm_set_temporal(s, C.byref(sp)) and L.sgm_reset(s, w, h, C.byref(opt))
    L.stub_clear()
    L.stub_temporal_clear_log()
    return s, opt


def images(batch=1, w=W, h=H):
    shape = (batch, h, w)
    return np.zeros(shape, np.uint8), np.ones(shape, np.uint8), np.full(shape, -1, np.float32)


def kinds(L):
    return [L.stub_temporal_kind(i) for i in range(L.stub_temporal_count())]


def test_spec_validation_at_every_range_edge(host, capfd):
    import soc_project_stereo_matching_amd as S
    s = host.sgm_create(0)
    good = dict(alpha=0.4, delta=1.0, hold_window=3, hold_count=2, sequence=0, min_conf=0, stats=0)
    edges_ok = [dict(alpha=1.0), dict(alpha=1e-45), dict(delta=0.0), dict(delta=3.4e38), dict(hold_window=0, hold_count=0),
                dict(hold_window=0, hold_count=99), dict(hold_window=8, hold_count=8), dict(hold_window=8, hold_count=1), dict(sequence=1),
                dict(min_conf=65535), dict(stats=1)]
    edges_bad = [dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=np.nextafter(np.float32(1), np.float32(2))), dict(alpha=float("nan")),
                 dict(alpha=float("inf")), dict(delta=-1e-45), dict(delta=float("nan")), dict(delta=float("inf")), dict(hold_window=-1),
                 dict(hold_window=9, hold_count=1), dict(hold_window=3, hold_count=0), dict(hold_window=3, hold_count=4), dict(sequence=2),
                 dict(sequence=-1), dict(min_conf=65536), dict(stats=2), dict(stats=-1)]
    for kw in edges_ok:
        sp = S.SGMTemporalSpec(**dict(good, **kw))
        assert host.sgm_set_temporal(s, C.byref(sp)) and host.SGM_SetTemporal(C.byref(sp)), kw
    for kw in edges_bad:
        sp = S.SGMTemporalSpec(**dict(good, **kw))
        assert not host.sgm_set_temporal(s, C.byref(sp)) and not host.SGM_SetTemporal(C.byref(sp)), kw
    assert "temporal spec is outside its ranges" in capfd.readouterr().err
    assert host.sgm_set_temporal(s, None) and host.SGM_SetTemporal(None) and not host.sgm_set_temporal(None, None)
    # the standalone filter: the same ranges but sequence and stats, which it does not look at; geometry; pointers
    host.stub_temporal_clear_log()
    m, hv, hb = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint8)
    conf, st = np.zeros(8, np.uint16), np.zeros(10, np.uint32)
    call = lambda sp, streams=1, steps=2, pixels=4, maps=m.ctypes.data, k=conf.ctypes.data, v=hv.ctypes.data, b=hb.ctypes.data, c=st.ctypes.data, inst=s: \
        host.sgm_temporal_filter(inst, None if sp is None else C.byref(sp), streams, steps, pixels, maps, k, v, b, c)
    assert call(S.SGMTemporalSpec(**dict(good, sequence=7, stats=-3))) and host.stub_temporal_count() == 1
    p = host.stub_temporal_params(0).contents
    assert (p.a, p.b, p.delta, p.n, p.k, p.min_conf) == (np.float32(0.4), np.float32(1) - np.float32(0.4), 1.0, 3, 2, 0)
    assert [host.stub_temporal_geometry(0, i) for i in range(3)] == [1, 2, 4]
    assert call(S.SGMTemporalSpec(**good), k=None, c=None) and host.stub_temporal_count() == 2
    ok = S.SGMTemporalSpec(**good)
    for kw in edges_bad[:12] + [dict(min_conf=65536)]:
        assert not call(S.SGMTemporalSpec(**dict(good, **kw))), kw
    assert not call(None) and not call(ok, inst=None) and not call(ok, maps=None) and not call(ok, v=None) and not call(ok, b=None)
    assert not call(ok, streams=0) and not call(ok, steps=0) and not call(ok, pixels=0)
    assert not call(ok, streams=1 << 31, steps=1, pixels=2) and not call(ok, streams=3, steps=1 << 30, pixels=1)
    assert not call(ok, streams=1 << 40, steps=1 << 40, pixels=1 << 40)
    assert not call(ok, maps=m.ctypes.data + 2) and not call(ok, v=hv.ctypes.data + 1) and not call(ok, k=conf.ctypes.data + 1)
    assert not host.sgm_temporal_clear(s, 0, 4, hv.ctypes.data, hb.ctypes.data) and not host.sgm_temporal_clear(s, 1, 4, None, hb.ctypes.data)
    assert not host.sgm_temporal_clear(s, 1 << 20, 1 << 20, hv.ctypes.data, hb.ctypes.data)
    assert host.stub_temporal_count() == 2                        # refusals queue nothing
    assert host.sgm_temporal_clear(s, 2, 4, hv.ctypes.data, hb.ctypes.data) and kinds(host) == [0, 0, 1]
    assert np.all(np.isposinf(hv)) and not hb.any() and host.stub_temporal_geometry(2, 2) == 8
    host.sgm_destroy(s)
    host.SGM_Shutdown()


def test_never_set_logs_what_a_build_without_the_feature_logs(host, host_without):
    """allocations and their sizes included: an instance that never sets a temporal spec is the instance it was"""
    left, right, out = images()
    conf = np.zeros((H, W), np.uint16)
    logs = []
    host.stub_temporal_clear_log()
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = option()
        L.stub_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_both(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        L.sgm_destroy(s)
    assert logs[0] == logs[1]
    assert host.stub_temporal_count() == 0
    # set and taken back before it took effect: still nothing
    s = host.sgm_create(0)
    opt = option()
    sp = c_spec(GOOD)
    assert host.sgm_set_temporal(s, C.byref(sp)) and host.sgm_set_temporal(s, None)
    host.stub_clear()
    assert host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
    assert [(e.name, e.arg) for e in standin.log(host)] == logs[0][:len(standin.log(host))] and host.stub_temporal_count() == 0
    host.sgm_destroy(s)


@pytest.mark.parametrize("overlap", [0, 1])
def test_one_more_launch_behind_the_median_on_the_post_stream(host, overlap):
    left, right, out = images()
    s, opt = make(host)
    assert host.sgm_set_overlap_post(s, overlap)
    host.stub_clear()
    assert host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
    assert kinds(host) == [1, 0]                                  # the first filtered match clears, then filters: nothing else
    names = [e.name for e in standin.log(host)]
    med = names.index("median")
    assert host.stub_temporal_at(0) == host.stub_temporal_at(1) == med + 1                # right behind the median
    assert "d2h" in names[med + 1:] and not set(names[med + 1:]) & {"speckle", "lrcheck", "sum_wta_lr", "aggregate"}
    on_main = host.stub_temporal_stream(1) == host.sgm_stream(s)
    assert on_main == (not overlap) and host.stub_temporal_stream(0) == host.stub_temporal_stream(1)
    assert [host.stub_temporal_geometry(1, i) for i in range(3)] == [1, 1, W * H] and host.stub_temporal_geometry(0, 2) == W * H
    assert host.stub_temporal_ptr(1, 1) is None and host.stub_temporal_ptr(1, 4)          # min_conf == 0: no confidence; stats on
    # the filtered map is what the caller gets: the stand-in's maps are 0 -> class "first", out 0, counted
    st = np.zeros((1, 5), np.uint32)
    assert not out.any() and host.sgm_temporal_stats(s, st.ctypes.data, 1) == 1 and st.tolist() == [[W * H, 0, 0, 0, 0]]
    assert host.sgm_temporal_stats(s, st.ctypes.data, 0) == 0
    # behind the refinement where that is on
    assert host.sgm_set_refine(s, 1, 16.0, 1.5, 1, 0) and host.sgm_reset(s, W, H, C.byref(opt))
    host.stub_clear()
    host.stub_temporal_clear_log()
    assert host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data) and kinds(host) == [0]
    names = [e.name for e in standin.log(host)]
    last_refine = max(i for i, n in enumerate(names) if n == "refine_pass")
    assert host.stub_temporal_at(0) == last_refine + 1
    host.sgm_destroy(s)


def test_history_survives_reset_and_each_restart_rule_clears_once(host):
    left, right, out = images()
    s, opt = make(host)
    match = lambda: host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)

    def after(change=None):
        host.stub_temporal_clear_log()
        if change:
            change()
        assert match() and match()
        return kinds(host)

    st = np.zeros((2, 5), np.uint32)
    assert after() == [1, 0, 0]                                   # the first match; then Reset keeps the history
    assert host.sgm_temporal_stats(s, st.ctypes.data, 2) == 1 and st[0].tolist() == [0, W * H, 0, 0, 0]      # smoothed: it was kept
    assert after() == [0, 0]
    assert after(lambda: host.sgm_temporal_restart(s)) == [1, 0, 0]
    sp = c_spec(GOOD, 0, 1)
    assert after(lambda: host.sgm_set_temporal(s, C.byref(sp))) == [1, 0, 0]              # the same spec again
    assert after(lambda: host.sgm_set_reference_view(s, 1)) == [1, 0, 0]
    assert after(lambda: host.sgm_set_reference_view(s, 0)) == [1, 0, 0]
    # a shape change and back
    assert host.sgm_reset(s, W + 2, H, C.byref(opt))
    l2, r2, o2 = images(w=W + 2)
    host.stub_temporal_clear_log()
    assert host.sgm_match(s, l2.ctypes.data, r2.ctypes.data, o2.ctypes.data) and kinds(host) == [1, 0]
    assert after() == [1, 0, 0]
    # plain -> both -> plain
    host.stub_temporal_clear_log()
    both = lambda: host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match_both(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, o2.ctypes.data)
    assert both() and both() and kinds(host) == [1, 0, 0]
    assert [host.stub_temporal_geometry(1, i) for i in range(3)] == [2, 1, W * H] and host.stub_temporal_geometry(0, 2) == 2 * W * H
    assert host.sgm_temporal_stats(s, st.ctypes.data, 2) == 2 and host.sgm_temporal_stats(s, st.ctypes.data, 1) == 0
    assert after() == [1, 0, 0]
    # a batch change; sequence mode is one stream of B steps
    sq = c_spec(GOOD, 1, 1)
    assert host.sgm_set_batch(s, 3) and host.sgm_set_temporal(s, C.byref(sq))
    l3, r3, o3 = images(3)
    host.stub_temporal_clear_log()
    for _ in range(2):
        assert host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match(s, l3.ctypes.data, r3.ctypes.data, o3.ctypes.data)
    assert kinds(host) == [1, 0, 0] and [host.stub_temporal_geometry(1, i) for i in range(3)] == [1, 3, W * H]
    assert host.stub_temporal_geometry(0, 2) == W * H
    st3 = np.zeros((3, 5), np.uint32)
    assert host.sgm_temporal_stats(s, st3.ctypes.data, 3) == 3 and st3[:, 1].tolist() == [W * H] * 3
    # off again: nothing more is launched
    assert host.sgm_set_temporal(s, None)
    host.stub_temporal_clear_log()
    assert host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match(s, l3.ctypes.data, r3.ctypes.data, o3.ctypes.data) and kinds(host) == []
    assert host.sgm_temporal_stats(s, st3.ctypes.data, 3) == 0
    host.sgm_destroy(s)


def test_stage_read_back_of_the_history(host):
    left, right, out = images(2)
    s, opt = make(host, batch=2)
    host.sgm_keep_stages(s, 1)
    got = np.zeros((H, W), np.float32)
    bits = np.zeros((H, W), np.uint8)
    assert host.sgm_read_stage(s, 30, got.ctypes.data, got.nbytes) == 0                  # nothing filtered yet
    assert host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
    for which, buf in ((29, got), (30, got), (31, bits)):
        assert host.sgm_read_stage(s, which, buf.ctypes.data, buf.nbytes) == buf.nbytes, which
    assert not got.any() and np.all(bits == 1)
    assert host.sgm_read_stage(s, 33, got.ctypes.data, got.nbytes) == 0 and host.sgm_read_stage(s, 32, got.ctypes.data, got.nbytes) == 0
    assert host.sgm_match_both(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, out.copy().ctypes.data)
    for which, buf in ((29, got), (30, got), (31, bits), (32, got), (33, got), (34, bits)):
        assert host.sgm_read_stage(s, which, buf.ctypes.data, buf.nbytes) == buf.nbytes, which
    assert np.all(got == 2.0) and np.all(bits == 1)                                        # the stand-in's right maps are 2.0
    host.sgm_destroy(s)


def test_a_refused_launch_fails_the_match_and_leaves_the_history(host, capfd):
    left, right, out = images()
    s, opt = make(host)
    match = lambda: host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
    hv, hb = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint8)

    def history():
        assert host.sgm_read_stage(s, 30, hv.ctypes.data, hv.nbytes) and host.sgm_read_stage(s, 31, hb.ctypes.data, hb.nbytes)
        return hv.tobytes() + hb.tobytes()

    assert match() and match()
    before = history()
    assert np.all(hb == 3)
    host.stub_temporal_clear_log()
    host.stub_temporal_fail_at(0)
    assert not match() and "a kernel launch failed" in capfd.readouterr().err
    assert kinds(host) == [0] and history() == before
    st = np.zeros((1, 5), np.uint32)
    assert host.sgm_temporal_stats(s, st.ctypes.data, 1) == 0    # the failed match counted nothing
    assert match() and kinds(host) == [0, 0] and np.all(np.frombuffer(history()[-W * H:], np.uint8) == 7)
    # a failure earlier in the match: the filter is not reached
    host.stub_temporal_clear_log()
    host.stub_fail_at(b"median", 0)
    assert not match() and kinds(host) == [] and match() and kinds(host) == [0]
    # a refused clear: the restart is still owed
    assert host.sgm_temporal_restart(s)
    host.stub_temporal_clear_log()
    host.stub_temporal_fail_at(0)
    assert not match() and kinds(host) == [1] and match() and kinds(host) == [1, 1, 0]
    # an allocation that fails at initialize
    assert host.sgm_set_batch(s, 2)
    host.stub_fail_at(b"alloc", 0)
    assert not host.sgm_reset(s, W, H, C.byref(opt))
    capfd.readouterr()
    host.sgm_destroy(s)


def test_row_tiles_refuse_and_a_build_without_the_stub_answers_false(host, host_without, capfd):
    s, opt = make(host)
    assert host.sgm_set_rows(s, 0, H // 2) and not host.sgm_reset(s, W, H, C.byref(opt))
    assert "temporal filter (sgm_set_temporal) works on whole frames" in capfd.readouterr().err
    assert host.sgm_set_temporal(s, None) and host.sgm_reset(s, W, H, C.byref(opt))
    host.sgm_destroy(s)
    s = host_without.sgm_create(0)
    sp = c_spec(GOOD)
    m, hv, hb = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint8)
    assert not host_without.sgm_set_temporal(s, C.byref(sp)) and not host_without.SGM_SetTemporal(C.byref(sp))
    assert not host_without.sgm_temporal_filter(s, C.byref(sp), 1, 1, 4, m.ctypes.data, None, hv.ctypes.data, hb.ctypes.data, None)
    assert not host_without.sgm_temporal_clear(s, 1, 4, hv.ctypes.data, hb.ctypes.data)
    assert capfd.readouterr().err.count("the temporal filter is not part of this build") == 4
    assert host_without.sgm_set_temporal(s, None) and host_without.sgm_temporal_restart(s)
    assert host_without.sgm_temporal_stats(s, m.ctypes.data, 1) == 0
    host_without.sgm_destroy(s)


def test_min_conf_adds_the_confidence_launchers_and_zero_does_not(host, tmp_path):
    left, right, out = images()
    conf = np.zeros((H, W), np.uint16)
    names = {}
    for min_conf in (0, 20000):
        s, opt = make(host, GOOD._replace(min_conf=min_conf))
        assert host.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        names[min_conf] = [e.name for e in standin.log(host)]
        given = host.stub_temporal_ptr(1, 1)
        assert (given is not None) == (min_conf > 0)
        if min_conf:
            assert standin.calls(host, "sum_wta_lr_conf")[0].a == given           # the internal map the cost sum wrote
            # the caller's map where one is given
            host.stub_clear()
            host.stub_temporal_clear_log()
            assert host.sgm_reset(s, W, H, C.byref(opt)) and host.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, conf.ctypes.data)
            assert standin.calls(host, "sum_wta_lr_conf")[0].a == host.stub_temporal_ptr(0, 1)
            # both views: the confidence is one view's
            assert not host.sgm_match_both(s, left.ctypes.data, right.ctypes.data, out.ctypes.data, out.copy().ctypes.data)
        host.sgm_destroy(s)
    assert "sum_wta_lr_conf" in names[20000] and "sum_wta_lr" not in names[20000]
    assert "sum_wta_lr" in names[0] and "sum_wta_lr_conf" not in names[0]
    # a build with the filter and without the confidence kernels refuses min_conf > 0 only
    L = _sign(standin.build(tmp_path, without=("conf",), extra_sources=[STUB_TEMPORAL], flags=("-ffp-contract=off",)))
    s = L.sgm_create(0)
    sp0, sp1 = c_spec(GOOD), c_spec(GOOD._replace(min_conf=1))
    assert L.sgm_set_temporal(s, C.byref(sp0)) and not L.sgm_set_temporal(s, C.byref(sp1))
    L.sgm_destroy(s)


def test_default_instance_remembers_the_spec_across_shutdown(host):
    left, right, out = images()
    opt = option()
    sp = c_spec(GOOD, 0, 1)
    st = np.zeros((1, 5), np.uint32)
    assert not host.SGM_TemporalRestart() and host.SGM_TemporalStats(st.ctypes.data, 1) == 0
    assert host.SGM_SetTemporal(C.byref(sp))
    for _ in range(2):
        host.stub_temporal_clear_log()
        assert host.SGM_Reset(W, H, C.byref(opt)) and host.SGM_Match(left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert host.SGM_Reset(W, H, C.byref(opt)) and host.SGM_Match(left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert kinds(host) == [1, 0, 0] and host.SGM_TemporalStats(st.ctypes.data, 1) == 1 and st[0, 1] == W * H
        assert host.SGM_TemporalRestart()
        host.SGM_Shutdown()
    assert host.SGM_SetTemporal(None)
    host.stub_temporal_clear_log()
    assert host.SGM_Reset(W, H, C.byref(opt)) and host.SGM_Match(left.ctypes.data, right.ctypes.data, out.ctypes.data) and kinds(host) == []
    host.SGM_Shutdown()


# ---- sanitizers on a stand-alone program -----------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_temporal_host_is_asan_ubsan_clean(tmp_path):
    """tests/temporal_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in filter."""
    exe = standin.build(tmp_path, sanitize=True, exe="temporal_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "temporal_sanitize_driver.c"), STUB_TEMPORAL])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("temporal_sanitize_driver ok")
