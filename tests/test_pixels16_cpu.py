"""Images of 9..16 bits per sample (extension; the contract is in include/sgm_mi355x.h, SGM_SetPixelBits) without a GPU: the numpy
restatement (tests/pixels16_ref.py) against hand-worked windows and, on 8-bit content, against the oracle's own census; the two
identities the GPU tests rest on, shown on the restatement; the C host's logic on the stand-in device (tests/stub_device.c +
tests/stub_pixels16.c, whose launchers compute for real); the Python wrapper's dtype checks; a sanitizer run of a stand-alone
driver."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pixels16_ref as P
import rectify_ref as RR
import standin
from conftest import ROOT, load_npz

STUB_P16 = os.path.join(ROOT, "tests", "stub_pixels16.c")
STUB_RECTIFY = os.path.join(ROOT, "tests", "stub_rectify.c")
_p, _i, _b = C.c_void_p, C.c_int, C.c_bool


def noise16(w, h, seed=1, frames=None, top=65536):
    shape = (h, w) if frames is None else (frames, h, w)
    return np.random.default_rng(seed).integers(0, top, shape, dtype=np.uint16)


# ---- the restatement: hand-worked windows --------------------------------------------------------------------------------------

def test_narrowing_shifts_and_saturates():
    v = np.array([[0, 15, 16, 4095, 4096, 65535]], np.uint16)
    assert P.narrow(v, 12).tolist() == [[0, 0, 1, 255, 255, 255]]        # >= 2^12 saturates
    assert P.narrow(v, 16).tolist() == [[0, 0, 0, 15, 16, 255]]
    assert P.narrow(v, 9).tolist() == [[0, 7, 8, 255, 255, 255]]
    for bits in range(9, 17):
        u8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
        assert np.array_equal(P.narrow(P.widen(u8, bits), bits), u8)


def test_centre_census_of_a_hand_worked_5x5_window():
    """6x6 so that the window fits (W > 5 and H > 5); the one interior-by-rule pixel set is rows 2..3 x columns 2..3.  Pixel (2, 2):
    the window is rows 0..4 x columns 0..4; samples below the centre value 1000 sit at raster positions 0, 6, 24 of 25."""
    img = np.full((6, 6), 2000, np.uint16)
    img[2, 2] = 1000
    img[0, 0], img[1, 1], img[4, 4] = 999, 0, 998                       # raster positions 0, 6, 24
    img[2, 3] = 1000                                                   # equal: strict <, counts as 0
    got = P.census_centre(img)
    assert got.dtype == np.uint32
    assert int(got[2, 2]) == (1 << 24) | (1 << 18) | 1
    assert not got[:2].any() and not got[4:].any() and not got[:, :2].any() and not got[:, 4:].any()
    # differences the 8-bit image does not have: 999 and 1000 are one grey level at 12 bits
    assert int(P.census_centre(P.narrow(img, 12))[2, 2]) == (1 << 18)   # 998, 999 and 1000 are all 62 there; only the 0 is below


def test_symmetric_census_of_a_hand_worked_3x3_window():
    """3x3: n = 4 pairs (-1,-1)|(1,1), (-1,0)|(1,0), (-1,1)|(1,-1), (0,-1)|(0,1), first pair in the highest bit."""
    img = np.array([[10, 500, 30, 7],
                    [40000, 9, 39999, 7],
                    [31, 499, 11, 7],
                    [7, 7, 7, 7]], np.uint16)
    got = P.census_sym(img, 3, 3)
    # pixel (1, 1): 10 < 11 -> 1, 500 < 499 -> 0, 30 < 31 -> 1, 40000 < 39999 -> 0
    assert int(got[1, 1]) == 0b1010
    assert got[0].tolist() == [0] * 4 and got[:, 0].tolist() == [0] * 4 and got[3].tolist() == [0] * 4


def test_wide_centre_census_word_is_u64_with_the_first_comparison_on_top():
    img = np.full((10, 12), 300, np.uint16)
    img[1, 1] = 299                                                    # first sample of the 9x7 window of pixel (4, 5)
    img[7, 9] = 0                                                      # its last sample
    got = P.census_centre(img, 9, 7)
    assert got.dtype == np.uint64 and int(got[4, 5]) == (1 << 62) | 1
    assert not P.census_centre(img[:7], 9, 7).any()                    # H == ch: the window does not fit


@pytest.mark.parametrize("w,h", [(70, 33), (20, 31), (5, 9)])
def test_on_8_bit_content_the_restatement_is_the_oracles_census(oracle, w, h):
    img = np.random.default_rng(w).integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(P.census_centre(img), oracle.census(img))
    for cw, ch in ((7, 7), (9, 7), (3, 21)):
        assert np.array_equal(P.census_centre(img, cw, ch), oracle.census_window(img, cw, ch))
    import census_sym_ref as CS
    assert np.array_equal(P.census_sym(img, 7, 7), CS.census_sym(img, 7, 7))
    mx, my = RR.model_maps(RR.SMALL, w, h)
    assert np.array_equal(P.remap(img, mx, my), RR.remap(img, mx, my))


def test_remap_keeps_all_16_bits():
    w, h = 40, 24
    img = noise16(w, h, 3)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    assert np.array_equal(P.remap(img, x, y), img)                       # identity maps reproduce the image
    full = np.full((h, w), 65535, np.uint16)
    got = P.remap(full, x + 0.46875, y + 0.28125)                        # 15/32 and 9/32: every weight in play
    assert np.all(got[:h - 1, :w - 1] == 65535)                          # 1024 * 65535 + 512 >> 10
    half = P.remap(img, x + 0.5, y)
    p00 = img.astype(np.int64)
    p01 = np.concatenate([p00[:, 1:], np.zeros((h, 1), np.int64)], axis=1)
    assert np.array_equal(half, ((p00 + p01 + 1) >> 1).astype(np.uint16))


# ---- the two identities of the GPU tests, on the restatement --------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    z = load_npz("tiny_t70x33_d16.npz")
    return z["left"], z["right"]


@pytest.mark.parametrize("bits", [9, 12, 16])
def test_shift_identity(tiny, bits):
    for img in tiny:
        v = P.widen(img, bits)
        assert np.array_equal(P.narrow(v, bits), img)
        assert np.array_equal(P.census_centre(v), P.census_centre(img))
        assert np.array_equal(P.census_centre(v, 9, 7), P.census_centre(img, 9, 7))
        assert np.array_equal(P.census_sym(v, 7, 7), P.census_sym(img, 7, 7))


@pytest.mark.parametrize("bits", [12, 16])
def test_rank_identity_and_that_the_low_bits_matter(tiny, bits):
    l16, r16 = P.lut_pair(*tiny, bits, seed=bits)
    assert l16.dtype == np.uint16 and int(max(l16.max(), r16.max())) < (1 << bits)
    rl, rr = P.rank_pair(l16, r16)
    for a, b in ((l16, rl), (r16, rr)):
        assert np.array_equal(P.census_centre(a), P.census_centre(b))
        assert np.array_equal(P.census_sym(a, 9, 7), P.census_sym(b, 9, 7))
        assert np.array_equal(P.census_centre(a, 7, 7), P.census_centre(b, 7, 7))
    # tone-mapped to 8 bits the census loses comparisons: the content exercises the low bits
    assert not np.array_equal(P.census_centre(P.narrow(l16, bits)), P.census_centre(l16))


# ---- the interface ---------------------------------------------------------------------------------------------------------------

def test_python_wrapper_and_header():
    import soc_project_stereo_matching_amd as S
    lib = S.load_library()
    for sym in ("SGM_SetPixelBits", "sgm_set_pixel_bits", "sgmd_census16", "sgmd_remap16"):
        assert hasattr(lib, sym), sym
    for cls in (S.SGM, S.SGMInstance):
        assert callable(getattr(cls, "set_pixel_bits", None)) and callable(getattr(cls, "read_narrowed", None))
    assert (S.STAGE_NARROW_LEFT, S.STAGE_NARROW_RIGHT) == (21, 22)
    assert "narrow" not in " ".join(S.STAGE_NAMES)                     # read_stages() is what it was
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    assert re.search(r"bool\s+SGM_SetPixelBits\(int bits\);", text) and re.search(r"bool\s+sgm_set_pixel_bits\(sgm_instance\* s, int bits\);", text)
    assert "g8 = min(v >> (bits - 8), 255)" in text and "1024 * 65535 + 512 < 2^32" in text
    # the ABI is unchanged: the match entry points still take const uint8_t*
    assert re.search(r"bool SGM_Match\(const uint8_t\* img_left, const uint8_t\* img_right, float\* disp_left\);", text)
    # refusals need no device
    assert not lib.SGM_SetPixelBits(7) and not lib.SGM_SetPixelBits(17) and not lib.SGM_SetPixelBits(-1) and lib.SGM_SetPixelBits(8)


def test_wrapper_checks_the_dtype_against_the_bits_in_effect():
    """Without a device: an instance object whose C handle is never used -- the checks come before the call."""
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance.__new__(S.SGMInstance)
    i.handle, i.shape, i.batch = None, (4, 6, 8), 1
    a8, a16, out = np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint16), np.zeros((4, 6), np.float32)
    with pytest.raises(TypeError):
        i.match(a16, a16)                                              # 8 bits in effect: uint16 would be read as half the rows
    with pytest.raises(TypeError):
        i.match_async(a16, a16, out)
    i._bits = 12
    for call in (lambda: i.match(a8, a8), lambda: i.match_confidence(a8, a8), lambda: i.match_both(a8, a8),
                 lambda: i.match_async(a8, a8, out), lambda: i.match(a16.astype(np.int16), a16.astype(np.int16)),
                 lambda: i.match_confidence_async(a8, a8, out, np.zeros((4, 6), np.uint16)),
                 lambda: i.match_both_async(a8, a8, out, out.copy())):
        with pytest.raises(TypeError):
            call()
    g = S.SGM.__new__(S.SGM)
    g._bits = 12
    for call in (lambda: g.match(a8, a8), lambda: g.match_confidence(a8, a8), lambda: g.match_both(a8, a8)):
        with pytest.raises(TypeError):
            call()
    i.handle = None                                                    # (close() of the never-created handle does nothing)


def test_default_instance_bits_are_shared_by_every_sgm_object():
    """The default instance and its bits are one per process in C: a second SGM object, or one made after set_pixel_bits, must
    check dtypes against the same width, and a compute() whose C call fails must leave the width in effect as it was."""
    import soc_project_stereo_matching_amd as S
    a = S.SGM()
    try:
        assert a.set_pixel_bits(12)
        b = S.SGM()
        assert (b._bits_req, b._bits) == (12, 8) and not b.set_pixel_bits(17) and b._bits_req == 12
        a8 = np.zeros((4, 6), np.uint8)
        with pytest.raises(TypeError):
            b.compute(a8, a8, S.default_option(8))                     # compute resets first: the 12 bits asked for hold for it
        empty = np.zeros((0, 0), np.uint16)
        assert b.compute(empty, empty, S.default_option(8)) is None    # refused by the C side before any device is touched
        assert (S.SGM._bits_req, S.SGM._bits, a._bits) == (12, 8, 8)
        with pytest.raises(TypeError):
            a.match(empty, empty)                                      # still 8 bits in effect
    finally:
        assert a.set_pixel_bits(8)
    assert S.SGM()._bits_req == 8


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

def _sign(L):
    for name, (res, args) in {"sgm_set_pixel_bits": (_b, [_p, _i]), "SGM_SetPixelBits": (_b, [_i]),
                              "sgm_set_rectify": (_b, [_p, _i, _i] + [_p] * 4), "sgm_rectify": (_b, [_p] * 5),
                              "sgm_set_census_kind": (_b, [_p, _i]), "sgm_set_census_window": (_b, [_p, _i, _i]),
                              "sgm_match_planes": (_b, [_p, _p, C.c_float, C.c_float, C.c_float, _p]),
                              "sgm_select_frame": (None, [_p, _i]),
                              "SGM_Initialize": (_b, [C.c_uint16, C.c_uint16, _p]), "SGM_Reset": (_b, [C.c_uint16, C.c_uint16, _p]),
                              "SGM_Match": (_b, [_p] * 3), "SGM_Shutdown": (None, []),
                              "stub_p16_ptr": (_p, [_i, _i]), "stub_p16_count": (_i, []), "stub_p16_arg": (_i, [_i, _i]),
                              "stub_p16_fail_at": (None, [_i]), "stub_p16_clear": (None, []),
                              "stub_remap_count": (_i, [])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("p16stub"), extra_sources=[STUB_P16, STUB_RECTIFY], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("p16stub_without")))


W, H = 65, 17                      # odd: a batch's second frame starts at an odd sample
KIND, BITS, SYM, CW, CH, FRAMES, AT = range(7)


def make(L, bits=None):
    import soc_project_stereo_matching_amd as S
    s = L.sgm_create(0)
    assert s
    if bits is not None:
        assert L.sgm_set_pixel_bits(s, bits)
    return s, S.default_option(16)


def device(ptr, n, dtype):
    n_bytes = n * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * n_bytes).from_address(ptr), dtype).copy()


def census_calls(L):
    return [k for k in range(L.stub_p16_count()) if L.stub_p16_arg(k, KIND) == 0]


def args(*arrays):
    return tuple(a.ctypes.data for a in arrays)


@pytest.mark.parametrize("bits,sym,cw,ch", [(12, 0, 5, 5), (16, 0, 5, 5), (10, 1, 7, 7), (12, 0, 9, 7), (9, 1, 5, 5)])
def test_match_uploads_u16_and_the_census_writes_words_and_narrowed_images(host, bits, sym, cw, ch):
    L = host
    s, opt = make(L, bits)
    assert L.sgm_set_census_kind(s, sym) and L.sgm_set_census_window(s, cw, ch) and L.sgm_reset(s, W, H, C.byref(opt))
    left, right = noise16(W, H, 5), noise16(W, H, 6)                   # samples >= 2^bits among them
    out = np.zeros((H, W), np.float32)
    L.stub_clear(); L.stub_p16_clear()
    assert L.sgm_match(s, *args(left, right, out))
    # the uploads are 2 * px bytes each
    assert [e.arg for e in standin.log(L) if e.name == "h2d"] == [2 * W * H, 2 * W * H]
    calls = census_calls(L)
    assert len(calls) == 1 and L.stub_p16_count() == 1
    k = calls[0]
    assert [L.stub_p16_arg(k, f) for f in (BITS, SYM, CW, CH, FRAMES)] == [bits, sym, cw, ch, 1]
    src_l, src_r, cl, cr, gl, gr = (L.stub_p16_ptr(k, j) for j in range(6))
    assert np.array_equal(device(src_l, W * H, np.uint16).reshape(H, W), left)
    assert np.array_equal(device(src_r, W * H, np.uint16).reshape(H, W), right)
    word = np.uint64 if (not sym and (cw, ch) != (5, 5)) else np.uint32
    assert np.array_equal(device(cl, W * H, word).reshape(H, W), P.census(left, sym, cw, ch))
    assert np.array_equal(device(cr, W * H, word).reshape(H, W), P.census(right, sym, cw, ch))
    assert np.array_equal(device(gl, W * H, np.uint8).reshape(H, W), P.narrow(left, bits))
    assert np.array_equal(device(gr, W * H, np.uint8).reshape(H, W), P.narrow(right, bits))
    # no 8-bit census launch beside it; the wide centre window still materialises its cost volume
    names = [n for n, _ in standin.launches(L)]
    assert "census" not in names and "census_window" not in names
    assert ("cost64" in names and "aggregate_volume" in names) == (word is np.uint64)
    # stages 0 / 1 and 21 / 22 read what the census wrote
    got = np.zeros((H, W), word)
    assert L.sgm_read_stage(s, 0, got.ctypes.data, got.nbytes) == got.nbytes and np.array_equal(got, P.census(left, sym, cw, ch))
    g8 = np.zeros((H, W), np.uint8)
    assert L.sgm_read_stage(s, 22, g8.ctypes.data, g8.nbytes) == g8.nbytes and np.array_equal(g8, P.narrow(right, bits))
    assert L.sgm_read_stage(s, 21, g8.ctypes.data, g8.nbytes - 1) == 0
    L.sgm_destroy(s)


def test_downstream_reads_the_narrowed_images(host):
    """The stand-in's toy aggregation and cost sum compute from the image they are handed: with v = u8 << 4 the 12-bit match must
    produce the 8-bit match's map, which it only does if the aggregation was handed g8 (not the u16 samples read as bytes)."""
    L = host
    w, h = 24, 8
    img = np.random.default_rng(2).integers(0, 256, (h, w), dtype=np.uint8)
    maps = []
    L.stub_toy_compute(1)
    try:
        for bits in (8, 12):
            s, opt = make(L, bits)
            assert L.sgm_reset(s, w, h, C.byref(opt))
            a = img if bits == 8 else P.widen(img, bits)
            out = np.zeros((h, w), np.float32)
            assert L.sgm_match(s, *args(a, a.copy(), out))
            maps.append(out)
            L.sgm_destroy(s)
    finally:
        L.stub_toy_compute(0)
    assert maps[0].any() and np.array_equal(maps[0], maps[1])


def test_order_remap_census_guide_copy_and_the_guide_is_the_narrowed_image(host):
    L = host
    s, opt = make(L, 12)
    mx, my = RR.model_maps(RR.SMALL, W, H)
    m = [np.ascontiguousarray(a, np.float32) for a in (mx, my, mx, my)]
    assert L.sgm_set_rectify(s, W, H, *args(*m)) and L.sgm_set_refine(s, 1, 16.0, 1.5, 1, 0) and L.sgm_reset(s, W, H, C.byref(opt))
    left, right = noise16(W, H, 7, top=4096), noise16(W, H, 8, top=4096)
    out = np.zeros((H, W), np.float32)
    for right_view in (0, 1):
        L.sgm_set_reference_view(s, right_view)
        L.stub_clear(); L.stub_p16_clear()
        assert L.sgm_match(s, *args(left, right, out))
        assert L.stub_remap_count() == 0                                # the 8-bit remap is not used
        kinds = [L.stub_p16_arg(k, KIND) for k in range(L.stub_p16_count())]
        assert kinds == [1, 0]                                          # remap16, then census16
        rect_l, rect_r = L.stub_p16_ptr(0, 3), L.stub_p16_ptr(0, 4)
        assert (L.stub_p16_ptr(1, 0), L.stub_p16_ptr(1, 1)) == (rect_l, rect_r)     # the census reads the rectified images
        assert np.array_equal(device(rect_l, W * H, np.uint16).reshape(H, W), P.remap(left, mx, my))
        # the guide copy is queued behind the census: the first d2d of W * H bytes in the main log comes after the census call
        log = standin.log(L)
        at = L.stub_p16_arg(1, AT)
        copies = [k for k, e in enumerate(log) if e.name == "d2d" and e.arg == W * H]
        assert copies and copies[0] >= at
        guide = standin.calls(L, "refine_pass")[0].b
        g8 = L.stub_p16_ptr(1, 5 if right_view else 4)
        assert np.array_equal(device(guide, W * H, np.uint8), device(g8, W * H, np.uint8))
        assert np.array_equal(device(g8, W * H, np.uint8).reshape(H, W), P.narrow(P.remap(right if right_view else left, mx, my), 12))
        # stages 19 / 20 are u16 now
        got = np.zeros((H, W), np.uint16)
        assert L.sgm_read_stage(s, 20, got.ctypes.data, got.nbytes) == got.nbytes and np.array_equal(got, P.remap(right, mx, my))
        assert L.sgm_read_stage(s, 19, got.ctypes.data, W * H) == 0     # the 8-bit capacity is too small
    # the stand-alone remap follows the instance's bits
    ol, orr = np.zeros_like(left), np.zeros_like(right)
    assert L.sgm_rectify(s, *args(left, right, ol, orr))
    assert np.array_equal(ol, P.remap(left, mx, my)) and np.array_equal(orr, P.remap(right, mx, my))
    assert not L.sgm_rectify(s, left.ctypes.data + 1, right.ctypes.data, ol.ctypes.data, orr.ctypes.data)
    L.sgm_destroy(s)


def test_batch_of_three_with_odd_frames(host):
    L = host
    s, opt = make(L, 16)
    assert L.sgm_set_batch(s, 3) and L.sgm_reset(s, W, H, C.byref(opt))
    left, right = noise16(W, H, 9, frames=3), noise16(W, H, 10, frames=3)
    out = np.zeros((3, H, W), np.float32)
    L.stub_clear(); L.stub_p16_clear()
    assert L.sgm_match(s, *args(left, right, out))
    assert [e.arg for e in standin.log(L) if e.name == "h2d"] == [2 * 3 * W * H] * 2
    assert L.stub_p16_count() == 1 and L.stub_p16_arg(0, FRAMES) == 3
    words = device(L.stub_p16_ptr(0, 3), 3 * W * H, np.uint32).reshape(3, H, W)
    for f in range(3):
        assert np.array_equal(words[f], P.census_centre(right[f]))
    L.sgm_select_frame(s, 1)
    g8 = np.zeros((H, W), np.uint8)
    assert L.sgm_read_stage(s, 21, g8.ctypes.data, g8.nbytes) == g8.nbytes and np.array_equal(g8, P.narrow(left[1], 16))
    L.sgm_destroy(s)


def test_8_bits_launch_and_allocate_what_a_host_without_the_feature_does(host, host_without):
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out = np.zeros((H, W), np.float32)
    logs = []
    for L, set8 in ((host, True), (host, False), (host_without, True)):
        s, opt = make(L, 8 if set8 else None)
        L.stub_clear()
        if hasattr(L, "stub_p16_clear"):
            L.stub_p16_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, *args(left, right, out))
        logs.append([(e.name, e.arg) for e in standin.log(L)])          # allocations and their sizes included
        g8 = np.zeros((H, W), np.uint8)
        assert L.sgm_read_stage(s, 21, g8.ctypes.data, g8.nbytes) == 0 and L.sgm_read_stage(s, 22, g8.ctypes.data, g8.nbytes) == 0
        L.sgm_destroy(s)
    assert logs[0] == logs[1] == logs[2] and host.stub_p16_count() == 0


def test_every_refusal_queues_nothing(host, host_without):
    L = host
    s, opt = make(L)
    left, right = noise16(W, H, 1), noise16(W, H, 2)
    out = np.zeros((H, W), np.float32)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    # bad values change nothing: the instance stays initialized at 8 bits
    for bad in (7, 17, -1, 0, 255):
        assert not L.sgm_set_pixel_bits(s, bad) and not L.SGM_SetPixelBits(bad), bad
    assert not L.sgm_set_pixel_bits(None, 12)
    l8 = np.zeros((H, W), np.uint8)
    L.stub_clear(); L.stub_p16_clear()
    assert L.sgm_match(s, *args(l8, l8, out)) and L.stub_p16_count() == 0 and ("census", 1) in standin.launches(L)
    # a change of bits asks for a new initialize; then: planes, odd device addresses, row tiles
    assert L.sgm_set_pixel_bits(s, 12) and not L.sgm_match(s, *args(left, right, out))
    assert L.sgm_reset(s, W, H, C.byref(opt))
    planes, depth = np.zeros((6, H, W), np.uint8), np.zeros((H, W), np.float32)
    conf = np.zeros((H, W), np.uint16)
    L.stub_clear(); L.stub_p16_clear()
    assert not L.sgm_match_planes(s, planes.ctypes.data, 700.0, 160.0, 0.0, depth.ctypes.data)
    for l, r in ((left.ctypes.data + 1, right.ctypes.data), (left.ctypes.data, right.ctypes.data + 1)):
        assert not L.sgm_match_device(s, l, r, out.ctypes.data)
        assert not L.sgm_match_confidence_device(s, l, r, out.ctypes.data, conf.ctypes.data)
        assert not L.sgm_match_both_device(s, l, r, out.ctypes.data, depth.ctypes.data)
    assert standin.log(L) == [] and L.stub_p16_count() == 0
    assert L.sgm_match_device(s, *args(left, right, out)) and L.stub_p16_count() == 1      # 2-byte alignment is enough
    assert L.sgm_set_rows(s, 4, 12)
    L.stub_clear(); L.stub_p16_clear()
    assert not L.sgm_reset(s, W, H, C.byref(opt)) and not L.sgm_initialize(s, W, H, C.byref(opt))
    assert standin.launches(L) == [] and L.stub_p16_count() == 0
    assert L.sgm_set_pixel_bits(s, 8) and L.sgm_reset(s, W, H, C.byref(opt))               # row tiles with 8 bits: as ever
    L.sgm_destroy(s)
    # a host linked without the launchers: 8 is accepted, 9..16 are not, and nothing changes
    L = host_without
    s, opt = make(L)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    for bits in range(9, 17):
        assert not L.sgm_set_pixel_bits(s, bits) and not L.SGM_SetPixelBits(bits)
    assert L.sgm_set_pixel_bits(s, 8) and L.SGM_SetPixelBits(8)
    L.stub_clear()
    assert L.sgm_match(s, *args(l8, l8, out)) and ("census", 1) in standin.launches(L)     # still initialized
    L.sgm_destroy(s)


def test_a_refused_census_launch_abandons_the_match(host):
    L = host
    s, opt = make(L, 12)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    left, right = noise16(W, H, 1), noise16(W, H, 2)
    out = np.zeros((H, W), np.float32)
    L.stub_clear(); L.stub_p16_clear()
    L.stub_p16_fail_at(0)
    assert not L.sgm_match(s, *args(left, right, out))
    assert not [n for n, _ in standin.launches(L) if n.startswith(("aggregate", "sum_wta"))]
    L.stub_p16_clear()
    assert L.sgm_match(s, *args(left, right, out)) and L.stub_p16_count() == 1
    L.sgm_destroy(s)


def test_one_instance_through_8_12_8_bits_and_changing_shapes(host):
    L = host
    s, opt = make(L)
    fresh, _ = make(L)
    out = np.zeros((40, 80), np.float32)

    def run(inst, w, h, bits):
        assert L.sgm_set_pixel_bits(inst, bits) and L.sgm_reset(inst, w, h, C.byref(opt))
        dt = np.uint16 if bits > 8 else np.uint8
        a, b = (np.random.default_rng(k).integers(0, 200, (h, w)).astype(dt) for k in (1, 2))
        L.stub_clear(); L.stub_p16_clear()
        assert L.sgm_match(inst, *args(a, b, out))
        uploads = [e.arg for e in standin.log(L) if e.name == "h2d"]
        assert uploads == [w * h * np.dtype(dt).itemsize] * 2
        assert L.stub_p16_count() == (1 if bits > 8 else 0)
        return standin.launches(L)

    first = run(s, W, H, 8)
    run(s, W, H, 12)
    assert run(s, W, H, 8) == first == run(fresh, W, H, 8)               # back at 8 bits: the launches of a fresh instance
    run(s, 80, 40, 12)                                                  # grows with 12 bits in effect
    run(s, 20, 9, 16)                                                   # shrinks
    assert run(s, W, H, 8) == first
    L.sgm_destroy(s)
    L.sgm_destroy(fresh)


def test_default_instance_remembers_the_bits_across_shutdown(host):
    L = host
    import soc_project_stereo_matching_amd as S
    opt = S.default_option(16)
    left, right = noise16(W, H, 3), noise16(W, H, 4)
    out = np.zeros((H, W), np.float32)
    assert L.SGM_SetPixelBits(12)
    try:
        L.stub_p16_clear()
        assert L.SGM_Initialize(W, H, C.byref(opt)) and L.SGM_Match(*args(left, right, out)) and L.stub_p16_count() == 1
        L.SGM_Shutdown()
        assert L.SGM_Reset(W, H, C.byref(opt)) and L.SGM_Match(*args(left, right, out)) and L.stub_p16_count() == 2
        assert L.stub_p16_arg(1, BITS) == 12
        assert np.array_equal(device(L.stub_p16_ptr(1, 2), W * H, np.uint32).reshape(H, W), P.census_centre(left))
        assert L.SGM_SetPixelBits(8)
        l8 = np.zeros((H, W), np.uint8)
        assert L.SGM_Reset(W, H, C.byref(opt)) and L.SGM_Match(*args(l8, l8, out)) and L.stub_p16_count() == 2
    finally:
        L.SGM_SetPixelBits(8)
        L.SGM_Shutdown()


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_pixels16_host_is_asan_ubsan_clean(tmp_path):
    """tests/pixels16_sanitize_driver.c: a program of its own, linked with the host and the stubs."""
    exe = standin.build(tmp_path, sanitize=True, exe="pixels16_sanitize_driver", flags=("-ffp-contract=off",),
                        extra_sources=[os.path.join(ROOT, "tests", "pixels16_sanitize_driver.c"), STUB_P16, STUB_RECTIFY])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("pixels16_sanitize_driver ok")
