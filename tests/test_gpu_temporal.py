"""The temporal filter on the device (include/sgm_mi355x.h, sgm_temporal_spec; csrc/sgm_temporal.hip) -- needs an MI355X.

Parity unpinned by the reference (it treats every frame as the only one): expected results are tests/temporal_ref.py, for the kernel
alone on the random inputs of tests/temporal_cases.py (whose class coverage tests/test_temporal_cpu.py asserts), and through the
match on the CPU oracle's final maps of six noisy frames per golden pair, pushed through the restatement in order.
Tolerance: 0 -- maps, history and counters are compared as bit patterns."""
import numpy as np
import pytest

import fill_holes_ref as F
import temporal_cases as TC
import temporal_ref as TR
from conftest import case_inputs, option_from_dict

pytestmark = pytest.mark.gpu


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={got[first]} reference={want[first]}")


def c_spec(spec, sequence=0, stats=1):
    import soc_project_stereo_matching_amd as S
    return S.SGMTemporalSpec(spec.alpha, spec.delta, spec.n, spec.k, sequence, spec.min_conf, stats)


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------

def device_copy(a, skip_bytes=0):
    """a device tensor holding `a` that starts skip_bytes into a fresh (256-byte aligned) allocation -> (the owner, the address)"""
    import torch
    raw = np.zeros(a.nbytes + 64, np.uint8)
    raw[skip_bytes:skip_bytes + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + skip_bytes


def host_copy(t, skip_bytes, like):
    return t.cpu().numpy()[skip_bytes:skip_bytes + like.nbytes].view(like.dtype).reshape(like.shape)


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    yield i
    i.close()


@pytest.mark.parametrize("k", range(len(TC.PARAMS)))
@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
def test_kernel_alone_equals_the_restatement(inst, shape, k):
    import torch
    spec = TC.PARAMS[k]
    pixels, streams, steps, misaligned = shape
    maps, conf, hv, hb = TC.inputs(shape, spec)
    sp = c_spec(spec)
    for with_conf in (True, False):
        want = TR.run(spec, maps, conf if with_conf else None, hv, hb)
        for with_stats in (True, False):
            what = f"{TC.shape_id(shape)} {spec} conf={with_conf} stats={with_stats}"
            d_maps, p_maps = device_copy(maps, 4 if misaligned else 0)
            d_conf, p_conf = device_copy(conf, 2 if misaligned else 0)
            d_hv, p_hv = device_copy(hv)
            d_hb, p_hb = device_copy(hb)
            d_st, p_st = device_copy(np.full((streams * steps, 5), 0xA5A5A5A5, np.uint32))
            torch.cuda.synchronize()
            assert inst.temporal_filter(sp, streams, steps, pixels, p_maps, p_conf if with_conf else None, p_hv, p_hb,
                                        p_st if with_stats else None), what
            assert inst.synchronize()
            assert_same(host_copy(d_maps, 4 if misaligned else 0, maps), want[0], what + ": maps")
            assert_same(host_copy(d_hv, 0, hv), want[1], what + ": hv")
            assert_same(host_copy(d_hb, 0, hb), want[2], what + ": hb")
            if with_stats:
                assert_same(host_copy(d_st, 0, want[3]), want[3], what + ": counters")
            # nothing behind the maps was written
            assert not d_maps.cpu().numpy()[(4 if misaligned else 0) + maps.nbytes:].any(), what


def test_clear_and_refusals(inst):
    import torch
    hv = torch.zeros(1001, dtype=torch.float32, device="cuda")
    hb = torch.full((1001,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert inst.temporal_clear(7, 143, hv.data_ptr(), hb.data_ptr()) and inst.synchronize()
    assert bool(torch.isposinf(hv).all()) and not bool(hb.any())
    sp = c_spec(TC.MATCH_SPEC)
    assert not inst.temporal_filter(sp, 0, 1, 143, hv.data_ptr(), None, hv.data_ptr(), hb.data_ptr())
    assert not inst.temporal_filter(sp, 1, 1, 143, hv.data_ptr() + 2, None, hv.data_ptr(), hb.data_ptr())
    assert not inst.temporal_filter(c_spec(TC.MATCH_SPEC._replace(alpha=0.0)), 1, 1, 143, hv.data_ptr(), None, hv.data_ptr(), hb.data_ptr())
    assert inst.synchronize() and bool(torch.isposinf(hv).all())


# ---- through the match ---------------------------------------------------------------------------------------------------------

SPEC = TC.MATCH_SPEC
_cache = {}


def sequence(oracle, golden_cases, name, right_view=False):
    """the six frames of a pair, the oracle's final map of each (of the right view with right_view), the restatement's rows"""
    key = (name, right_view)
    if key not in _cache:
        case = golden_cases[name]
        left, right = case_inputs(case, oracle)
        opt = option_from_dict(case["option"])
        frames = TC.frames_of(left, right)
        try:
            oracle.set_reference_view(right_view)
            finals = [oracle.run(l, r, opt)["final"] for l, r in frames]
        finally:
            oracle.set_reference_view(False)
        for f in finals:
            f.setflags(write=False)
        _cache[key] = (opt, frames, finals, TC.filtered(SPEC, finals))
    return _cache[key]


def make(batch=1, spec=SPEC, sequence_mode=0, stats=1, keep=True, **settings):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0, batch=batch)
    i.keep_stages(keep)
    assert i.set_temporal(c_spec(spec, sequence_mode, stats))
    for name, value in settings.items():
        assert getattr(i, name)(value) is not False, name
    return i


def check_state(i, row, what, right=False):
    hv, hb = i.read_temporal(right)
    assert_same(hv, row[1], what + ": hv")
    assert_same(hb, row[2], what + ": hb")


@pytest.mark.parametrize("name", TC.PAIRS)
def test_six_single_frame_calls_with_reset(oracle, golden_cases, name):
    opt, frames, finals, rows = sequence(oracle, golden_cases, name)
    h, w = finals[0].shape
    i = make()
    try:
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)                              # the per-frame Reset of a stream keeps the history
            got = i.match(l, r)
            assert got is not None
            what = f"{name} frame {k}"
            assert_same(i.read_stage(29), finals[k], what + ": stage 29 (the oracle's final, unchanged by the feature)")
            assert_same(got, rows[k][0], what + ": the returned map")
            assert_same(i.read_stage("final"), rows[k][0], what + ": stage 8")
            check_state(i, rows[k], what)
            assert_same(i.temporal_stats(), rows[k][3].reshape(1, 5), what + ": counters")
        total = sum(r[3] for r in rows)
        assert np.all(total >= 10), (name, total)                  # every class is exercised
    finally:
        i.close()


@pytest.mark.parametrize("name", TC.PAIRS)
def test_two_sequence_batches_of_three_equal_six_calls(oracle, golden_cases, name):
    opt, frames, finals, rows = sequence(oracle, golden_cases, name)
    h, w = finals[0].shape
    i = make(batch=3, sequence_mode=1)
    try:
        for call in range(2):
            part = frames[3 * call:3 * call + 3]
            assert i.reset(w, h, opt)
            got = i.match(np.stack([p[0] for p in part]), np.stack([p[1] for p in part]))
            assert got is not None
            for f in range(3):
                k = 3 * call + f
                i.select_frame(f)
                assert_same(i.read_stage(29), finals[k], f"{name} frame {k}: stage 29")
                assert_same(got[f], rows[k][0], f"{name} frame {k}: the returned map")
                check_state(i, rows[3 * call + 2], f"{name} call {call}, read through frame {f}")       # the one stream
            assert_same(i.temporal_stats(), np.stack([rows[3 * call + f][3] for f in range(3)]), f"{name} call {call}: counters")
    finally:
        i.close()


def test_batch_of_three_streams(oracle, golden_cases):
    """sequence = 0: the frames of a batch are streams of their own -- three differently seeded ones, two calls"""
    name = "t70x33_d16"
    case = golden_cases[name]
    left, right = case_inputs(case, oracle)
    opt = option_from_dict(case["option"])
    h, w = left.shape
    streams = [TC.frames_of(left, right, first=10 * s, count=2, blank=10 * s + 1 if s == 1 else -1) for s in range(3)]
    rows = [TC.filtered(SPEC, [oracle.run(l, r, opt)["final"] for l, r in frames]) for frames in streams]
    i = make(batch=3)
    try:
        for call in range(2):
            assert i.reset(w, h, opt)
            got = i.match(np.stack([streams[s][call][0] for s in range(3)]), np.stack([streams[s][call][1] for s in range(3)]))
            for s in range(3):
                i.select_frame(s)
                assert_same(got[s], rows[s][call][0], f"stream {s} call {call}")
                check_state(i, rows[s][call], f"stream {s} call {call}")
            assert_same(i.temporal_stats(), np.stack([rows[s][call][3] for s in range(3)]), f"call {call}: counters")
    finally:
        i.close()


@pytest.mark.parametrize("how", ["async", "device", "overlap_post", "confidence", "right_view", "no_stats_no_keep"])
def test_entry_points_and_streams(oracle, golden_cases, how):
    import torch
    import soc_project_stereo_matching_amd as S
    name = "t70x33_d16"
    right_view = how == "right_view"
    opt, frames, finals, rows = sequence(oracle, golden_cases, name, right_view)
    h, w = finals[0].shape
    plain = S.SGMInstance(0) if how == "confidence" else None
    i = make(stats=0 if how == "no_stats_no_keep" else 1, keep=how != "no_stats_no_keep")
    try:
        i.set_reference_view(right_view)
        if how == "overlap_post":
            assert i.set_overlap_post(True)
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)
            what = f"{how} frame {k}"
            if how == "async":
                got = np.empty((h, w), np.float32)
                assert i.match_async(l, r, got) and i.match_wait()
            elif how == "device":
                tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
                out = torch.empty((h, w), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                assert i.match_device(tl.data_ptr(), tr.data_ptr(), out.data_ptr()) and i.synchronize()
                got = out.cpu().numpy()
            elif how == "confidence":
                got, conf = i.match_confidence(l, r)
                assert plain.reset(w, h, opt)
                want_map, want_conf = plain.match_confidence(l, r)
                assert_same(conf, want_conf, what + ": the confidence is an unfiltered instance's")
                assert_same(want_map, finals[k], what + ": the unfiltered map")
            else:
                got = i.match(l, r)
            assert_same(got, rows[k][0], what)
            check_state(i, rows[k], what)
            if how == "no_stats_no_keep":
                assert i.temporal_stats() is None
        # the filter off again: the oracle's maps
        assert i.set_temporal(None) and i.reset(w, h, opt)
        assert_same(i.match(*frames[0]), finals[0], f"{how}: the filter off")
        assert i.temporal_stats() is None
    finally:
        i.close()
        if plain:
            plain.close()


def test_min_conf_counts_low_confidence_as_holes(oracle, golden_cases):
    """expected from the GPU's own confidence map (which tests/test_gpu_confidence.py pins), internal and the caller's"""
    import soc_project_stereo_matching_amd as S
    opt, frames, finals, _ = sequence(oracle, golden_cases, "t70x33_d16")
    h, w = finals[0].shape
    spec = SPEC._replace(min_conf=20000)
    plain = S.SGMInstance(0)
    i = make(spec=spec)
    try:
        confs = []
        for l, r in frames:
            assert plain.reset(w, h, opt)
            confs.append(plain.match_confidence(l, r)[1])
        rows = TC.filtered(spec, finals, confs)
        assert sum(int(((c < 20000) & np.isfinite(f)).sum()) for c, f in zip(confs, finals)) > 100      # the gate does something
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)
            if k % 2:
                got, conf = i.match_confidence(l, r)
                assert_same(conf, confs[k], f"frame {k}: the caller's confidence")
            else:
                got = i.match(l, r)
            assert_same(got, rows[k][0], f"min_conf frame {k}")
            check_state(i, rows[k], f"min_conf frame {k}")
            assert_same(i.temporal_stats(), rows[k][3].reshape(1, 5), f"min_conf frame {k}: counters")
        assert i.match_both(*frames[0]) is None                    # the confidence is one view's
    finally:
        i.close()
        plain.close()


@pytest.mark.parametrize("name", ["t70x33_d16", "cone"])
def test_both_views_each_with_a_history_of_its_own(oracle, golden_cases, name):
    opt, frames, finals_l, rows_l = sequence(oracle, golden_cases, name)
    _, _, finals_r, rows_r = sequence(oracle, golden_cases, name, True)
    h, w = finals_l[0].shape
    i = make()
    try:
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)
            got_l, got_r = i.match_both(l, r)
            what = f"{name} both frame {k}"
            assert_same(i.read_stage(29), finals_l[k], what + ": stage 29")
            assert_same(i.read_stage(32), finals_r[k], what + ": stage 32")
            assert_same(got_l, rows_l[k][0], what + ": left")
            assert_same(got_r, rows_r[k][0], what + ": right")
            assert_same(i.read_stage(28), rows_r[k][0], what + ": stage 28")
            check_state(i, rows_l[k], what + " left")
            check_state(i, rows_r[k], what + " right", right=True)
            assert_same(i.temporal_stats(), np.stack([rows_l[k][3], rows_r[k][3]]), what + ": counters")
    finally:
        i.close()


def test_behind_hole_filling(oracle, golden_cases):
    opt, frames, _, _ = sequence(oracle, golden_cases, "t70x33_d16")
    h, w = frames[0][0].shape
    filled = [F.expected(oracle.run(l, r, opt), opt, oracle)[2] for l, r in frames]
    rows = TC.filtered(SPEC, filled)
    i = make(set_fill_holes=True)
    try:
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)
            got = i.match(l, r)
            assert_same(i.read_stage(29), filled[k], f"fill frame {k}: stage 29")
            assert_same(got, rows[k][0], f"fill frame {k}")
            check_state(i, rows[k], f"fill frame {k}")
    finally:
        i.close()


def test_behind_the_refinement(oracle, golden_cases):
    """expected from the GPU's own refined map (stage 29; tests/test_gpu_refine.py pins it)"""
    opt, frames, _, _ = sequence(oracle, golden_cases, "t70x33_d16")
    h, w = frames[0][0].shape
    i = make()
    try:
        assert i.set_refine(True)
        hv, hb = TR.empty(1, h * w)
        for k, (l, r) in enumerate(frames):
            assert i.reset(w, h, opt)
            got = i.match(l, r)
            row = TC.filtered(SPEC, [i.read_stage(29)], hv=hv, hb=hb)[0]
            hv, hb = row[1].reshape(1, -1), row[2].reshape(1, -1)
            assert_same(got, row[0], f"refine frame {k}")
            check_state(i, row, f"refine frame {k}")
        assert np.isfinite(got).sum() > 0
    finally:
        i.close()


def test_match_scaled_filters_its_small_map(oracle):
    import soc_project_stereo_matching_amd as S
    from oracle.pyoracle import default_option
    w, h, d = 128, 64, 32
    left, right = oracle.synth_pair(w, h, d, 0x7E4D)
    frames = TC.frames_of(left, right, count=3, blank=-1)
    opt = default_option(d // 2)
    spec = S.scale_spec(w, h, 2)
    i = make()
    try:
        hv, hb = TR.empty(1, (h // 2) * (w // 2))
        for k, (l, r) in enumerate(frames):
            assert i.reset(w // 2, h // 2, opt)
            assert i.match_scaled(spec, l, r) is not None
            row = TC.filtered(SPEC, [i.read_stage(29)], hv=hv, hb=hb)[0]
            hv, hb = row[1].reshape(1, -1), row[2].reshape(1, -1)
            assert_same(i.read_stage("final"), row[0], f"scaled frame {k}: stage 8 of the small map")
            check_state(i, row, f"scaled frame {k}")
        assert row[3][1] > 0                                       # the third frame met a history
    finally:
        i.close()


def test_history_lifetime(oracle, golden_cases):
    """each restart rule starts from an empty history, and nothing else does"""
    opt, frames, finals, _ = sequence(oracle, golden_cases, "t70x33_d16")
    h, w = finals[0].shape
    other = golden_cases["t24x16_d8"]
    ol, orr = case_inputs(other, oracle)
    oopt = option_from_dict(other["option"])
    i = make()
    fresh = lambda st: st[:, 1:4].sum() == 0 and st[:, 0].sum() > 0
    try:
        def match(frame=0, both=False):
            assert i.reset(w, h, opt)
            got = (i.match_both if both else i.match)(*frames[frame])
            assert got is not None
            return i.temporal_stats()

        assert fresh(match()) and not fresh(match(1)) and not fresh(match(2))
        assert i.temporal_restart() and fresh(match()) and not fresh(match(1))
        assert i.set_temporal(c_spec(SPEC)) and fresh(match()) and not fresh(match(1))                  # the same spec again
        # a shape change and back
        assert i.reset(ol.shape[1], ol.shape[0], oopt) and i.match(ol, orr) is not None and fresh(i.temporal_stats())
        assert i.reset(ol.shape[1], ol.shape[0], oopt) and i.match(ol, orr) is not None and not fresh(i.temporal_stats())
        assert fresh(match()) and not fresh(match(1))
        # a switch of the reference view, and back
        i.set_reference_view(True)
        assert fresh(match()) and not fresh(match(1))
        i.set_reference_view(False)
        assert fresh(match()) and not fresh(match(1))
        # plain -> both -> plain
        st = match(0, both=True)
        assert st.shape == (2, 5) and fresh(st[:1]) and fresh(st[1:])
        st = match(1, both=True)
        assert not fresh(st[:1]) and not fresh(st[1:])
        assert fresh(match()) and not fresh(match(1))
        # a batch change
        assert i.set_batch(2) and i.reset(w, h, opt)
        pair = (np.stack([frames[0][0], frames[1][0]]), np.stack([frames[0][1], frames[1][1]]))
        assert i.match(*pair) is not None
        st = i.temporal_stats()
        assert fresh(st[:1]) and fresh(st[1:])
        assert i.reset(w, h, opt) and i.match(*pair) is not None and not fresh(i.temporal_stats()[:1])
        assert i.set_batch(1)
        assert fresh(match()) and not fresh(match(1))
        # the last of them continued the history it found: frame 1 behind frame 0
        assert_same(i.read_stage("final"), TC.filtered(SPEC, finals[:2])[1][0], "frame 1 behind frame 0")
    finally:
        i.close()


def test_default_instance(oracle, golden_cases):
    import soc_project_stereo_matching_amd as S
    opt, frames, finals, rows = sequence(oracle, golden_cases, "t70x33_d16")
    h, w = finals[0].shape
    g = S.SGM()
    try:
        assert g.set_temporal(c_spec(SPEC))
        for k in range(3):
            got = g.compute(*frames[k], opt)
            assert_same(got, rows[k][0], f"default instance frame {k}")
            assert_same(g.temporal_stats(), rows[k][3].reshape(1, 5), f"default instance frame {k}: counters")
        hv, hb = g.read_temporal()
        assert_same(hv, rows[2][1], "default instance: hv")
        assert g.temporal_restart()
        assert_same(g.compute(*frames[0], opt), rows[0][0], "default instance: after the restart")
    finally:
        assert g.set_temporal(None)
        g.shutdown()
