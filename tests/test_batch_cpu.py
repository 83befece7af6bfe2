"""Batches of 1 to 1024 frames without a GPU: the C host (csrc/sgm_host.c) on the stand-in device (tests/standin.py,
tests/stub_device.c) -- what sgm_set_batch admits, and that every buffer request, fill and copy of a batch of 1024 has exactly the
expected size in size_t --, the arithmetic of tests/batch_cases.py (segment thresholds, the median's bands, the batches whose cells
pass 2^32), and the CPU oracle alone on every case of that module: every frame keeps enough content to mean something.
tests/test_gpu_batch_large.py runs the same cases on the device."""
import collections
import ctypes as C

import numpy as np
import pytest

import batch_cases as BC
import instance_steps as IR
import scaled_cases as SC
import standin

CENSUS_FRONT_SLACK = (65535 + 512 + 8 + 63) // 64 * 64 * 4        # csrc/sgm_host.c, with SGM_MAX_DISPARITY_RANGE = 512
CENSUS_BACK_SLACK = 64
CAP = 1 << 20                                                     # what the stand-in really allocates and copies


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    L = standin.build(tmp_path_factory.mktemp("batchstub"))
    L.stub_log_bytes.restype, L.stub_log_bytes.argtypes = C.c_size_t, [C.c_int]
    L.sgm_select_frame.restype, L.sgm_select_frame.argtypes = None, [C.c_void_p, C.c_int]
    return L


def option(d, dmin=0):
    import soc_project_stereo_matching_amd as S
    return S.default_option(d + dmin, dmin)


def sized(L, *names):
    """(name, bytes as size_t) of the allocations, fills and copies in the log"""
    return [(L.stub_log_name(i).decode(), int(L.stub_log_bytes(i))) for i in range(L.stub_log_size())
            if L.stub_log_name(i).decode() in (names or ("alloc", "memset", "h2d", "d2h", "d2d"))]


def bytes_of(L, name):
    return [n for k, n in sized(L, name)]


@pytest.fixture
def inst(host):
    s = host.sgm_create(0)
    assert s
    yield s
    host.sgm_destroy(s)


def reset(L, s, w, h, opt):
    L.stub_clear()
    assert L.sgm_reset(s, w, h, C.byref(opt))


def match(L, s, w, h, batch):
    img = np.zeros((batch, h, w), np.uint8)
    out = np.zeros((batch, h, w), np.float32)
    L.stub_clear()
    assert L.sgm_match(s, img.ctypes.data, img.ctypes.data, out.ctypes.data)


# ---- the stand-in device -------------------------------------------------------------------------------------------------------

def test_set_batch_admits_1_to_1024_and_a_refusal_changes_nothing(host, inst):
    L, s = host, inst
    w, h = 16, 8
    assert L.sgm_set_batch(s, 3)
    reset(L, s, w, h, option(8))
    match(L, s, w, h, 3)
    before = sized(L)
    assert bytes_of(L, "h2d") == [3 * w * h] * 2
    for bad in (0, -1, BC.BATCH_MAX + 1):
        assert not L.sgm_set_batch(s, bad)
        L.stub_clear()
        out = np.zeros((3, h, w), np.float32)
        assert L.sgm_read_stage(s, 8, out.ctypes.data, out.nbytes) == w * h * 4      # still initialised (frame 0 of three)
        reset(L, s, w, h, option(8))
        assert bytes_of(L, "alloc") == [], bad                # nothing is re-sized
        match(L, s, w, h, 3)                                  # still three frames
        assert sized(L) == before, bad
    assert L.sgm_set_batch(s, BC.BATCH_MAX) and L.sgm_set_batch(s, 1)


def test_select_frame_outside_the_batch_is_ignored(host, inst):
    L, s = host, inst
    w, h, B = 8, 8, BC.BATCH_MAX                              # 1024 maps of 256 bytes: inside what the stand-in really allocates
    assert L.sgm_set_batch(s, B)
    reset(L, s, w, h, option(8))
    match(L, s, w, h, B)
    out = np.zeros((h, w), np.float32)

    def source(frame):
        L.sgm_select_frame(s, frame)
        L.stub_clear()
        assert L.sgm_read_stage(s, 8, out.ctypes.data, out.nbytes) == out.nbytes
        (e,) = standin.calls(L, "d2h")
        return e.b

    base = source(0)
    assert source(B - 1) - base == (B - 1) * w * h * 4
    assert source(B) - base == (B - 1) * w * h * 4            # ignored: still the last frame
    assert source(-1) - base == (B - 1) * w * h * 4
    assert source(5) - base == 5 * w * h * 4


def expected_allocations(w, h, d, B):
    """the device allocations of sgm_reset on a fresh instance: ensure_buffers and sgm_initialize of csrc/sgm_host.c; the median
    scratch as the stand-in sizes it (W * H * 4)"""
    dp = BC.padded_stride(d)
    px = B * w * h
    return ([px, px, 4 * px, CENSUS_FRONT_SLACK + 4 * px + CENSUS_BACK_SLACK] + [4 * px] * 8 + [512] +
            [B * 8 * h * w * dp, B * 4 * h * dp, w * h * 4])


def test_every_request_fill_and_copy_of_1024_frames_has_its_size(host, inst):
    L, s = host, inst
    w, h, d, B = 16, 8, 8, BC.BATCH_MAX                       # maps of 512 KiB: the stand-in's copies stay inside its allocations
    px = B * w * h
    assert L.sgm_set_batch(s, B)
    reset(L, s, w, h, option(d))
    got = collections.Counter(bytes_of(L, "alloc"))
    want = collections.Counter(expected_allocations(w, h, d, B))
    assert not want - got, (want - got, got)
    extra = got - want                                        # the two path tables: [H][cap] entries of 8 bytes, [H] counts
    assert sorted(extra.elements()) == [4 * h, 8 * h * 6] or (len(list(extra.elements())) == 2 and max(extra) <= 8 * h * 8), extra
    # zero-filled: the stand-in's median scratch, census-left, census-right with the slack in front of it
    assert sorted(bytes_of(L, "memset")) == [w * h * 4, 4 * px, CENSUS_FRONT_SLACK + 4 * px]
    match(L, s, w, h, B)
    assert bytes_of(L, "h2d") == [px, px]
    pieces = bytes_of(L, "d2h")                               # a pageable result of 512 KiB: two pieces
    assert len(pieces) == BC.result_chunks(w, h, B) == 2 and sum(pieces) == 4 * px and all(p % 4 == 0 for p in pieces)
    assert bytes_of(L, "alloc") == []
    # a match without Reset accumulates: S for the whole batch, zero-filled
    match(L, s, w, h, B)
    assert bytes_of(L, "alloc") == [2 * px * 32] and 2 * px * 32 in bytes_of(L, "memset")


def test_both_views_of_1024_frames(host, inst):
    L, s = host, inst
    w, h, d, B = 16, 8, 8, BC.BATCH_MAX
    px4 = B * w * h * 4
    assert L.sgm_set_batch(s, B)
    reset(L, s, w, h, option(d))
    img = np.zeros((B, h, w), np.uint8)
    out_l, out_r = np.zeros((B, h, w), np.float32), np.zeros((B, h, w), np.float32)
    L.stub_clear()
    assert L.sgm_match_both(s, img.ctypes.data, img.ctypes.data, out_l.ctypes.data, out_r.ctypes.data)
    allocs = collections.Counter(bytes_of(L, "alloc"))
    assert allocs[px4] >= 1 and allocs[2 * px4] >= 4, allocs   # the raw left map; both maps, labels, sizes, totals at 2 B
    (e,) = standin.calls(L, "lrcheck_both")
    assert e.arg >> 8 == B and e.b - e.a == px4               # the right view's maps start behind B left ones
    assert bytes_of(L, "d2h") == [px4, px4]
    assert (out_l == 1.0).all() and (out_r == 2.0).all()


def test_fused_sweep_scratch_of_1024_frames(host, monkeypatch):
    monkeypatch.setenv("SGM_UPSUM", "1")                      # read at sgm_create
    L = host
    s = L.sgm_create(0)
    try:
        w, h, d, B = 16, 8, 128, BC.BATCH_MAX
        assert L.sgm_set_batch(s, B)
        reset(L, s, w, h, option(d))
        match(L, s, w, h, B)
        assert L.sgm_fused_sweep_rows(s) == 3
        scratch = B * 6 * w * 128 + 4096                      # sgmd_upsum_scratch_bytes of tests/stub_device.c
        px = B * w * h                                        # (the kept copy of the left images, and its d2d)
        assert scratch > CAP and bytes_of(L, "alloc") == [scratch, px] and px in bytes_of(L, "d2d")
        (up,) = standin.calls(L, "upsum")
        fills = [(L.stub_log_ptr(i, 0), int(L.stub_log_bytes(i))) for i in range(L.stub_log_size()) if L.stub_log_name(i) == b"memset"]
        assert (up.a, scratch) in fills
    finally:
        L.sgm_destroy(s)


# ---- the arithmetic of tests/batch_cases.py ------------------------------------------------------------------------------------

def test_numbering_of_the_stage_batches():
    assert [BC.aggregation_numbering(b) for b in (1, 2, 3, 4, 8)] == ["plain", "strips", "plain", "strips", "plain"]
    assert all(BC.aggregation_numbering(b) == "plain" for b in BC.STAGE_BATCHES)
    assert set(BC.STAGE_BATCHES) == {5, 6, 7, 9, 16, 17}
    (w, h, _), (tw, th, _) = BC.STAGE_SHAPES
    assert w > h and tw < th


def test_segment_thresholds():
    w, h, d = BC.SEGMENT_SHAPE
    assert BC.sum_slots(BC.padded_stride(d)) == 2048
    choice = [BC.sum_segments(w, h, d, b) for b in range(1, BC.BATCH_MAX + 1)]
    last = {sg: max(b for b, (s, fb) in enumerate(choice, 1) if s == sg and not fb) for sg in (4, 3, 2, 1)}
    assert last == {4: 32, 3: 42, 2: 64, 1: 128}
    assert all(fb == (b > 128) for b, (s, fb) in enumerate(choice, 1))
    for sg, b in last.items():                                # both sides of every threshold, one B past the fallback
        assert b in BC.SEGMENT_BATCHES and b + 1 in BC.SEGMENT_BATCHES
    assert {b: BC.sum_segments(w, h, d, b) for b in BC.SEGMENT_BATCHES} == BC.SEGMENT_BATCHES


def test_result_pieces():
    w, h, _ = BC.MAX_SHAPE
    assert BC.result_chunks(w, h, BC.BATCH_MAX) == 2 and BC.result_chunks(w, h, 8) == 1
    w, h, _, b = BC.CHUNK_CASE
    assert BC.result_chunks(w, h, b) == BC.RESULT_CHUNKS and 4 * w * h * b >= BC.RESULT_CHUNK_SPLIT > 4 * w * h * (b - 1)


def test_bands_of_the_tall_case():
    w, h, d, B = BC.TALL_CASE
    assert BC.median_bands(514) == (8, 0) and BC.median_bands(300) == (5, 0)          # the serial kernel
    groups, nbands = BC.median_bands(h)
    assert (groups, nbands) == (9, 3)
    assert BC.CHAIN_RESIDENT_MAX == 2048 and nbands * (B - 1) <= BC.CHAIN_RESIDENT_MAX < nbands * B <= 3 * BC.BATCH_MAX


@pytest.mark.parametrize("name", list(BC.PAST32))
def test_totals_past_32_bits_by_arithmetic(name):
    """Sizes alone: the stand-in would really allocate the page-locked staging of such a batch."""
    w, h, d, B = BC.PAST32[name]
    cells = BC.past32_cells(name)
    assert cells < 2 ** 32 - 1 and B <= BC.BATCH_MAX          # admitted per frame (sgm_initialize), and as a batch
    assert B * cells > 2 ** 32
    if name == "fast":
        assert BC.padded_stride(d) == 128 and (B - 1) * cells <= 2 ** 32       # the smallest such batch
    else:
        assert BC.padded_stride(d) == 512
    sizes = BC.device_bytes(w, h, d, B)
    assert sizes["planes"] == 8 * B * cells > 2 ** 32 and ("S" in sizes) == (name == "dp512")
    if name == "dp512":
        assert sizes["S"] == 2 * B * cells and sizes["cost"] == B * cells
    need = BC.past32_need(name)
    assert 2 ** 35 < need < 2 ** 36 if name == "fast" else 2 ** 35 < need < 2 ** 36
    at = BC.past32_frame_of_cell(name)
    pair = lambda j: j % BC.PAST32_PAIRS
    assert at * cells <= 2 ** 32 < (at + 1) * cells and 0 < at <= B - 1
    assert pair(0) != pair(B - 1)
    around = [j for j in (at - 1, at, at + 1) if j <= B - 1]
    assert len({pair(j) for j in around}) == len(around) >= 2


# ---- the oracle alone: every case keeps enough content -------------------------------------------------------------------------

def quota(finals, what, right_view=True):
    for j, (final, disp_r) in enumerate(finals):
        assert BC.finite(final) >= BC.QUOTA, (what, j, BC.finite(final))
        if right_view:
            assert BC.finite(disp_r) >= BC.QUOTA, (what, j, BC.finite(disp_r))


def test_frames_of_a_batch_differ(oracle):
    w, h, d = BC.MAX_SHAPE
    _, L, R = BC.frames(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED)
    assert len({a.tobytes() for a in L}) == BC.BATCH_MAX and len({a.tobytes() for a in R}) == BC.BATCH_MAX
    maps = BC.finals(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED)
    assert len({m.tobytes() for m, _ in maps}) > BC.BATCH_MAX * 9 // 10


@pytest.mark.parametrize("shape", BC.STAGE_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_content_of_the_stage_cases(oracle, shape):
    w, h, d = shape
    for batch in BC.STAGE_BATCHES:
        quota(BC.finals(oracle, w, h, d, batch, BC.STAGE_SEED + 977 * batch + w), (shape, batch))


def test_content_of_the_segment_cases(oracle):
    w, h, d = BC.SEGMENT_SHAPE
    for batch in BC.SEGMENT_BATCHES:
        quota(BC.finals(oracle, w, h, d, batch, BC.SEGMENT_SEED + 977 * batch), ("segments", batch))


def test_content_of_the_maximum_the_pieces_and_the_walk(oracle):
    w, h, d = BC.MAX_SHAPE
    quota(BC.finals(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED), "1024 frames")
    quota(BC.finals(oracle, w, h, d, BC.BATCH_MAX, BC.MAX_SEED, True), "1024 frames, right view", right_view=False)
    cw, ch, cd, cb = BC.CHUNK_CASE
    quota(BC.finals(oracle, cw, ch, cd, cb, BC.CHUNK_SEED), "64 frames")
    for k, B in enumerate(BC.WALK_BATCHES):
        if B != BC.BATCH_MAX:
            quota(BC.finals(oracle, w, h, d, B, BC.WALK_SEED + 977 * k), ("walk", B))


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
@pytest.mark.parametrize("name", list(BC.VARIANTS))
def test_content_of_the_variants(oracle, name, batch):
    st = BC.variant_step(name, batch)
    opt = IR.option_of(st)
    seed = BC.VARIANT_SEED + 1009 * list(BC.VARIANTS).index(name) + 31 * batch
    pairs = BC.variant_frames(oracle, st, seed)[0]
    prev = BC.variant_frames(oracle, st, seed + 53)[0] if st["q14"] else None
    if prev:
        pairs, prev = prev, pairs
    for j, (l, r) in enumerate(pairs):
        want = IR.expected(oracle, st, opt, l, r, None if prev is None else prev[j])
        assert BC.finite(want["final"]) >= BC.QUOTA and BC.finite(want["disp_r"]) >= BC.QUOTA, (name, batch, j)


@pytest.mark.parametrize("batch", BC.VARIANT_BATCHES)
def test_content_of_the_temporal_scaled_and_tile_cases(oracle, batch):
    w, h, d = BC.TEMPORAL_SHAPE
    quota(BC.finals(oracle, w, h, d, batch, BC.VARIANT_SEED + 0x7E0 + batch), ("temporal", batch), right_view=False)
    w, h, d = BC.TILE_SHAPE
    quota(BC.finals(oracle, w, h, d, batch, BC.VARIANT_SEED + 0x711 + batch), ("tiles", batch), right_view=False)
    c = BC.scaled_case(batch)
    SC.composed_quotas(c, SC.composed(oracle, c))             # (asserts the quotas of tests/scaled_cases.py)


def test_content_of_the_tall_case(oracle):
    w, h, d, B = BC.TALL_CASE
    quota(BC.finals(oracle, w, h, d, B, BC.TALL_SEED), "tall")


def test_content_of_the_fused_sweep_cases(oracle):
    w, h, d = BC.FUSED_SHAPE
    assert BC.padded_stride(d) == 128 and w > h and w >= 64 and h >= 4            # sgmd_upsum_rows
    for batch in BC.FUSED_BATCHES:
        quota(BC.finals(oracle, w, h, d, batch, BC.FUSED_SEED + 977 * batch), ("fused", batch))


@pytest.mark.parametrize("name", list(BC.PAST32))
def test_content_of_the_pairs_past_32_bits(oracle, name):
    w, h, d, B = BC.PAST32[name]
    pairs = BC.past32_pairs(oracle, name)
    maps = [oracle.run(l, r, BC.option(d)) for l, r in pairs]
    for k, s in enumerate(maps):
        assert BC.finite(s["final"]) >= BC.QUOTA and BC.finite(s["disp_r"]) >= BC.QUOTA, (name, k)
    assert len({s["final"].tobytes() for s in maps}) == BC.PAST32_PAIRS                # four DISTINCT results
