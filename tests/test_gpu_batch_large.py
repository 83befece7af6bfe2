"""Batches past 8 frames on the device: 5 to 1024, every stage and entry point -- needs an MI355X.

sgm_set_batch admits 1 to 1024 frames per call; the block numbering of the aggregation, the segments per row of the fused cost sum,
the lanes per pixel, the speckle tiles and the median's grids depend on the batch alone, and sgm_match_both and the temporal filter
double it.  tests/batch_cases.py names each B and the branch it is there for, with the arithmetic that establishes it.  Every frame
of every batch has content of its own and is compared with that frame computed alone: the CPU oracle, and for what the reference
does not have the restatements the feature's own GPU test uses (tests/instance_steps.py, temporal_ref, tests/scaled_cases.py).
Tolerance 0, bit patterns.  tests/test_batch_cpu.py checks the cases on the oracle alone and the buffer sizes on the stand-in device."""
import numpy as np
import pytest

import batch_cases as BC
import confidence_ref as CR
import instance_steps as IR
import refine_ref as RF
import scaled_cases as SC
import temporal_cases as TC
from oracle.pyoracle import STAGE_NAMES
from test_gpu_instance_reuse import _tile, assert_same, new_instance, run_match

pytestmark = pytest.mark.gpu


def instance(batch, keep=False):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0, batch=batch)
    i.keep_stages(keep)
    return i


def check_maps(inst, got, want, what, right_view=True):
    """got [B][H][W] against want [(final, raw right view)] * B; the raw right view read back frame by frame"""
    assert got is not None and len(got) == len(want), what
    for j, (final, disp_r) in enumerate(want):
        assert_same(got[j], final, f"{what} frame {j}: final")
        if right_view:
            inst.select_frame(j)
            assert_same(inst.read_stage("disp_r"), disp_r, f"{what} frame {j}: raw right view")


# ---- a. every stage at the untested numberings ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", BC.STAGE_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
@pytest.mark.parametrize("batch", list(BC.STAGE_BATCHES))
def test_every_stage_of_every_frame(oracle, batch, shape):
    """keep_stages: all nine stages of every frame (the aggregation's plain numbering frame = blockIdx.x % B and its anomalous-line
    blocks frame + B * (dir - 4); W < H clears the diagonal planes)"""
    w, h, d = shape
    assert BC.aggregation_numbering(batch) == "plain"
    opt = BC.option(d)
    pairs, L, R = BC.frames(oracle, w, h, d, batch, BC.STAGE_SEED + 977 * batch + w)
    inst = instance(batch, keep=True)
    try:
        assert inst.reset(w, h, opt)
        out = inst.match(L, R)
        assert out is not None and out.shape == (batch, h, w)
        for j, (l, r) in enumerate(pairs):
            want = oracle.run(l, r, opt)
            inst.select_frame(j)
            got = inst.read_stages()
            for n in STAGE_NAMES:
                assert_same(got[n], want[n], f"B={batch} {w}x{h} frame {j}: {n}")
            assert_same(out[j], want["final"], f"B={batch} {w}x{h} frame {j}: result")
    finally:
        inst.close()


# ---- b. segment choice by batch alone ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", list(BC.SEGMENT_BATCHES))
def test_segments_of_the_fused_sum_follow_the_batch(oracle, monkeypatch, batch):
    """No kept S (it would force one segment), no SGM_SUM_SEGMENTS: the launcher's own choice, 4 / 3 / 2 / 1 segments and its
    fallback (tests/batch_cases.py, sum_segments)."""
    monkeypatch.delenv("SGM_SUM_SEGMENTS", raising=False)
    w, h, d = BC.SEGMENT_SHAPE
    assert BC.sum_segments(w, h, d, batch) == BC.SEGMENT_BATCHES[batch]
    seed = BC.SEGMENT_SEED + 977 * batch
    want = BC.finals(oracle, w, h, d, batch, seed)
    _, L, R = BC.frames(oracle, w, h, d, batch, seed)
    inst = instance(batch)
    try:
        assert inst.reset(w, h, BC.option(d))
        check_maps(inst, inst.match(L, R), want, f"B={batch} {w}x{h}")
    finally:
        inst.close()


# ---- c. the admitted maximum ---------------------------------------------------------------------------------------------------

def _max_inputs(oracle):
    w, h, d = BC.MAX_SHAPE
    return BC.frames(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED)


def _max_want(oracle, right_view=False):
    w, h, d = BC.MAX_SHAPE
    return BC.finals(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED, right_view)


@pytest.mark.parametrize("how", ["pageable", "pinned", "device", "both"])
def test_1024_frames(oracle, how):
    """B = 1024 at 24 x 16, D = 8, every frame against the oracle: host pointers on pageable arrays (the result comes back in two
    pieces) and on page-locked ones, device pointers (with kept stages: frame 1023 read back stage by stage), and both views
    (2048 maps: the post pass and the census grids run at 2 B)."""
    import torch
    w, h, d = BC.MAX_SHAPE
    B = BC.BATCH_MAX
    pairs, L, R = _max_inputs(oracle)
    want = _max_want(oracle)
    opt = BC.option(d)
    inst = instance(B, keep=(how == "device"))
    try:
        assert not inst.set_batch(B + 1) and inst.batch == B
        assert inst.reset(w, h, opt)
        if how == "pageable":
            assert BC.result_chunks(w, h, B) == 2
            check_maps(inst, inst.match(L, R), want, how)
        elif how == "pinned":
            hl, hr = inst.host_array(L.shape, np.uint8), inst.host_array(R.shape, np.uint8)
            out = inst.host_array(L.shape, np.float32)
            hl[:], hr[:], out[:] = L, R, -1.0
            assert inst.match_async(hl, hr, out) and inst.match_wait()
            check_maps(inst, out, want, how)
        elif how == "device":
            dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
            out = torch.full((B, h, w), -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert inst.match_device(dl.data_ptr(), dr.data_ptr(), out.data_ptr()) and inst.synchronize()
            check_maps(inst, out.cpu().numpy(), want, how)
            inst.select_frame(B - 1)
            inst.select_frame(B)                              # outside the batch: ignored
            stages = oracle.run(*pairs[B - 1], opt)
            for n in STAGE_NAMES[:-1]:                        # (after a device match the final map is in the caller's buffer)
                assert_same(inst.read_stage(n), stages[n], f"frame {B - 1}: {n}")
        else:
            got = inst.match_both(L, R)
            assert got is not None
            check_maps(inst, got[0], want, "both, left view")
            check_maps(inst, got[1], _max_want(oracle, True), "both, right view", right_view=False)
    finally:
        inst.close()


def test_64_frames_whose_pageable_result_comes_back_in_four_pieces(oracle):
    w, h, d, B = BC.CHUNK_CASE
    assert BC.result_chunks(w, h, B) == BC.RESULT_CHUNKS
    want = BC.finals(oracle, w, h, d, B, BC.CHUNK_SEED)
    _, L, R = BC.frames(oracle, w, h, d, B, BC.CHUNK_SEED)
    inst = instance(B)
    try:
        assert inst.reset(w, h, BC.option(d))
        check_maps(inst, inst.match(L, R), want, f"B={B} {w}x{h}")
    finally:
        inst.close()


# ---- d. variants in a batch ----------------------------------------------------------------------------------------------------

REFINE_ITERATIONS = 2


def _expected(oracle, st, opt, left, right, prev):
    """expected() of tests/instance_steps.py; the refinement with REFINE_ITERATIONS iterations instead of the default"""
    if not st["refine"]:
        return IR.expected(oracle, st, opt, left, right, prev)
    import soc_project_stereo_matching_amd as S
    want = IR.expected(oracle, dict(st, refine=False), opt, left, right, prev)
    conf = CR.confidence(want["aggr"], opt.min_disparity, st["view"])[3]
    tabs = RF.tables(S.REFINE_LAMBDA, S.REFINE_SIGMA, REFINE_ITERATIONS, S.load_library())
    want["final"] = RF.refine(want["final"], conf, right if st["view"] else left, tabs, False)
    return want


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
@pytest.mark.parametrize("name", list(BC.VARIANTS))
def test_variant_in_a_batch(oracle, monkeypatch, name, batch):
    st = BC.variant_step(name, batch)
    opt = IR.option_of(st)
    seed = BC.VARIANT_SEED + 1009 * list(BC.VARIANTS).index(name) + 31 * batch
    inst = new_instance(monkeypatch, {})
    try:
        IR.apply(inst, st)
        if st["refine"]:
            assert inst.set_refine(True, iterations=REFINE_ITERATIONS)
        tag = f"{name} B={batch}"
        assert inst.reset(st["w"], st["h"], opt), tag
        pairs, L, R = BC.variant_frames(oracle, st, seed)
        out = run_match(inst, st, L, R)
        prev = None
        if st["q14"]:
            prev = pairs
            pairs, L, R = BC.variant_frames(oracle, st, seed + 53)
            out = run_match(inst, st, L, R)
        for j, (l, r) in enumerate(pairs):
            want = _expected(oracle, st, opt, l, r, None if prev is None else prev[j])
            inst.select_frame(j)
            for key in ("final", "conf"):
                if key in want:
                    assert_same(out[key][j], want[key], f"{tag} frame {j}: {key}")
            assert_same(inst.read_stage("disp_r"), want["disp_r"], f"{tag} frame {j}: raw right view")
            assert_same(inst.read_stage("aggr"), want["aggr"], f"{tag} frame {j}: aggregated costs")
    finally:
        inst.close()


def _temporal_instance(batch, sequence):
    import soc_project_stereo_matching_amd as S
    sp = TC.MATCH_SPEC
    i = instance(batch, keep=True)
    assert i.set_temporal(S.SGMTemporalSpec(sp.alpha, sp.delta, sp.n, sp.k, sequence, sp.min_conf, 1))
    return i


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
def test_temporal_filter_one_stream_per_frame(oracle, batch):
    """sequence = 0: B streams, two calls; every stream has a pair of its own"""
    w, h, d = BC.TEMPORAL_SHAPE
    opt = BC.option(d)
    streams = [TC.frames_of(*oracle.synth_pair(w, h, d, BC.frame_seed(BC.VARIANT_SEED + 0x7E0 + batch, s)), first=10 * s, count=2, blank=-1)
               for s in range(batch)]
    rows = [TC.filtered(TC.MATCH_SPEC, [oracle.run(l, r, opt)["final"] for l, r in fr]) for fr in streams]
    i = _temporal_instance(batch, 0)
    try:
        for call in range(2):
            assert i.reset(w, h, opt)
            got = i.match(np.stack([streams[s][call][0] for s in range(batch)]), np.stack([streams[s][call][1] for s in range(batch)]))
            assert got is not None
            for s in range(batch):
                i.select_frame(s)
                hv, hb = i.read_temporal()
                assert_same(got[s], rows[s][call][0], f"B={batch} stream {s} call {call}")
                assert_same(hv, rows[s][call][1], f"B={batch} stream {s} call {call}: hv")
                assert_same(hb, rows[s][call][2], f"B={batch} stream {s} call {call}: hb")
            assert_same(i.temporal_stats(), np.stack([rows[s][call][3] for s in range(batch)]), f"B={batch} call {call}: counters")
        assert sum(int(rows[s][1][3][1]) for s in range(batch)) > 0          # the second call met a history
    finally:
        i.close()


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
def test_temporal_filter_sequence_batch(oracle, batch):
    """sequence = 1: the B frames of a call are consecutive frames of ONE stream"""
    w, h, d = BC.TEMPORAL_SHAPE
    opt = BC.option(d)
    frames = TC.frames_of(*oracle.synth_pair(w, h, d, BC.VARIANT_SEED + 0x5E0 + batch), count=batch, blank=2)
    finals = [oracle.run(l, r, opt)["final"] for l, r in frames]
    rows = TC.filtered(TC.MATCH_SPEC, finals)
    i = _temporal_instance(batch, 1)
    try:
        assert i.reset(w, h, opt)
        got = i.match(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
        assert got is not None
        for f in range(batch):
            i.select_frame(f)
            assert_same(i.read_stage(29), finals[f], f"B={batch} frame {f}: stage 29")
            assert_same(got[f], rows[f][0], f"B={batch} frame {f}: the returned map")
        hv, hb = i.read_temporal()
        assert_same(hv, rows[-1][1], f"B={batch}: hv")
        assert_same(hb, rows[-1][2], f"B={batch}: hb")
        assert_same(i.temporal_stats(), np.stack([r[3] for r in rows]), f"B={batch}: counters")
    finally:
        i.close()


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
def test_match_scaled_in_a_batch(oracle, batch):
    import soc_project_stereo_matching_amd as S
    c = BC.scaled_case(batch)
    W, H, f = c["W"], c["H"], c["f"]
    r = SC.composed(oracle, c)                                # (its quotas: tests/test_batch_cpu.py)
    inst = instance(batch)
    try:
        assert inst.reset(W // f, H // f, r["opt"])
        got = inst.match_scaled(S.scale_spec(W, H, f, frames=batch, radius=c["radius"]), r["left"], r["right"])
        assert got is not None
        for k in range(batch):
            assert_same(got.reshape(r["want"].shape)[k], r["want"][k], f"B={batch} frame {k}: the full map")
            inst.select_frame(k)
            assert_same(inst.read_stage(8), r["small"][k], f"B={batch} frame {k}: stage 8, the small map")
    finally:
        inst.close()


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
def test_row_tiles_of_a_batch_on_one_instance(oracle, monkeypatch, batch):
    """The top and the bottom tile of B frames on ONE instance, as test_row_tiles_of_one_frame_on_one_instance does it for one
    frame: the hand-over buffers carry the rows of all frames."""
    import torch
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")
    w, h, d = BC.TILE_SHAPE
    opt = BC.option(d)
    seed = BC.VARIANT_SEED + 0x711 + batch
    want = BC.finals(oracle, w, h, d, batch, seed)
    _, L, R = BC.frames(oracle, w, h, d, batch, seed)
    inst = new_instance(monkeypatch, {})
    try:
        assert inst.set_batch(batch)
        dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        disp, disp_b = (torch.zeros((batch, h, w), dtype=torch.float32, device="cuda") for _ in range(2))
        top, bottom = (0, h // 2), (h // 2, h)
        assert inst.set_rows(*top) and inst.reset(w, h, opt)
        fwd = torch.empty(inst.tile_boundary_bytes(), dtype=torch.uint8, device="cuda")
        bwd = torch.empty_like(fwd)
        assert not _tile(inst, top, w, h, opt, dl, dr, disp, {}, {True: fwd})
        assert inst.synchronize()
        assert _tile(inst, bottom, w, h, opt, dl, dr, disp_b, {True: fwd}, {False: bwd})
        assert _tile(inst, top, w, h, opt, dl, dr, disp, {False: bwd}, {})
        disp[:, h // 2:] = disp_b[:, h // 2:]
        torch.cuda.synchronize()
        assert inst.tile_post(disp.data_ptr()) and inst.synchronize()
        check_maps(inst, disp.cpu().numpy(), want, f"B={batch}: the gathered maps", right_view=False)
        assert inst.set_rows(0, 0) and inst.reset(w, h, opt)
        check_maps(inst, inst.match(L, R), want, f"B={batch}: a plain match after the tiles")
    finally:
        inst.close()


# ---- e. tall frames in a large batch -------------------------------------------------------------------------------------------

def test_chained_median_with_more_bands_than_fit_on_the_chip(oracle):
    """24 x 515: 9 groups of 64 interior rows, the chained median with 3 bands per frame; B = 683 gives 2049 bands, one more than
    256 CUs x 8 workgroups of 4 waves can hold at once, so a band may start before the band above it of the same frame has a slot
    and correctness rests on the ticket order.  Two matches on one instance (the second with the frames in
    reverse order): the generation of the granules advances."""
    w, h, d, B = BC.TALL_CASE
    assert BC.median_bands(h)[1] >= 2 and BC.median_bands(h)[1] * B > BC.CHAIN_RESIDENT_MAX
    inst = instance(B)
    try:
        want = BC.finals(oracle, w, h, d, B, BC.TALL_SEED)
        _, L, R = BC.frames(oracle, w, h, d, B, BC.TALL_SEED)
        for rep in range(2):                                  # the second match: the same frames in reverse order
            if rep:
                want, L, R = want[::-1], np.ascontiguousarray(L[::-1]), np.ascontiguousarray(R[::-1])
            assert inst.reset(w, h, BC.option(d))
            check_maps(inst, inst.match(L, R), want, f"match {rep}", right_view=(rep == 1))
    finally:
        inst.close()


# ---- f. the opt-in fused sweep -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", BC.FUSED_BATCHES)
def test_fused_sweep_in_a_batch(oracle, monkeypatch, batch):
    """SGM_UPSUM=1 at an eligible shape (W > H, Dp = 128, eight paths): the hand-over rows, progress words and tickets of B frames.
    A stalled hand-over ends at the kernel's own poll limit and a failed match."""
    w, h, d = BC.FUSED_SHAPE
    seed = BC.FUSED_SEED + 977 * batch
    want = BC.finals(oracle, w, h, d, batch, seed)
    _, L, R = BC.frames(oracle, w, h, d, batch, seed)
    inst = new_instance(monkeypatch, {"SGM_UPSUM": "1"})
    try:
        assert inst.set_batch(batch) and inst.reset(w, h, BC.option(d))
        got = inst.match(L, R)
        assert inst.fused_sweep_rows() > 0
        check_maps(inst, got, want, f"fused sweep B={batch}")
    finally:
        inst.close()


# ---- g. batch totals past 2^32 cells -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BC.PAST32))
def test_batch_totals_past_32_bits(oracle, name):
    """B * W * H * Dp passes 2^32 while every frame stays below it: every frame base has to be 64-bit arithmetic.  Four pairs cycle
    through the batch (frame j holds pair j % 4); every frame is compared with its pair's maps."""
    import torch
    w, h, d, B = BC.PAST32[name]
    assert BC.past32_cells(name) < 2 ** 32 - 1 < 2 ** 32 < B * BC.past32_cells(name)
    need = BC.past32_need(name)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{name}: needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")
    opt = BC.option(d)
    pairs = BC.past32_pairs(oracle, name)
    want = [oracle.run(l, r, opt) for l, r in pairs]
    L = np.stack([pairs[j % BC.PAST32_PAIRS][0] for j in range(B)])
    R = np.stack([pairs[j % BC.PAST32_PAIRS][1] for j in range(B)])
    inst = instance(B)
    try:
        assert inst.reset(w, h, opt)
        got = inst.match(L, R)
        assert got is not None
        for j in range(B):
            k = j % BC.PAST32_PAIRS
            assert_same(got[j], want[k]["final"], f"{name} frame {j} (pair {k}): final")
            inst.select_frame(j)
            assert_same(inst.read_stage("disp_r"), want[k]["disp_r"], f"{name} frame {j} (pair {k}): raw right view")
        at = BC.past32_frame_of_cell(name)
        for j in sorted({0, max(at - 1, 0), min(at, B - 1), min(at + 1, B - 1), B - 1}):     # S of the frames around cell 2^32
            inst.select_frame(j)
            assert_same(inst.read_stage("aggr"), want[j % BC.PAST32_PAIRS]["aggr"], f"{name} frame {j}: aggregated costs")
    finally:
        inst.close()


# ---- h. one instance through B = 17, 5, 1024, 2 --------------------------------------------------------------------------------

def test_one_instance_through_batches(oracle):
    """The batch counterpart of test_shape_ladder: one instance, one shape, the batch grows, shrinks, jumps to the maximum (every
    buffer is re-allocated) and ends on the XCD strips of two frames."""
    w, h, d = BC.WALK_SHAPE
    inst = instance(1)
    try:
        for k, B in enumerate(BC.WALK_BATCHES):
            seed = BC.MAX_SEED if B == BC.BATCH_MAX else BC.WALK_SEED + 977 * k
            want = BC.finals(oracle, w, h, d, B, seed)
            _, L, R = BC.frames(oracle, w, h, d, B, seed)
            assert inst.set_batch(B) and inst.reset(w, h, BC.option(d))
            check_maps(inst, inst.match(L, R), want, f"step {k}, B={B}")
            inst.select_frame(B - 1)
            l, r = BC.frames(oracle, w, h, d, B, seed)[0][B - 1]
            assert_same(inst.read_stage("aggr"), oracle.run(l, r, BC.option(d))["aggr"], f"step {k}, B={B}: S of the last frame")
    finally:
        inst.close()
