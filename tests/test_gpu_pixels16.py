"""Images of 9..16 bits per sample (SGM_SetPixelBits, include/sgm_mi355x.h) on an MI355X, through the C-ABI.  Parity unpinned by
the reference; tolerance 0 everywhere.  Three checks cover the path, with no golden data of their own:

  shift identity   u16 = u8 << (bits - 8): g8 == u8 and the census words are those of u8, so EVERY stage must equal the 8-bit match
                   of u8 -- the oracle's (adaptive P2 included), or, for an option the oracle does not chain, the 8-bit match of an
                   instance configured the same way (which the existing GPU tests pin).
  rank identity    v = lut[u8] with a random strictly increasing 12- / 16-bit lut (tests/pixels16_ref.py, lut_pair): a genuinely
                   16-bit pair with at most 256 distinct values.  Its dense ranks are a u8 pair with the same order relations, hence
                   the same census words; with p2_init <= p1 the P2 table is the constant P1 and grey values drop out.  So every
                   stage must equal the 8-bit match of the rank images bit for bit.  Where the census window fits the frame the test
                   also asserts that the 8-bit match of the narrowed pair g8 DIFFERS: the content exercises the low bits (in a frame
                   the window does not fit, all words are 0 on both sides and nothing can differ).
  stages           arbitrary random u16 content, samples >= 2^bits included: stages 0 / 1 (census words, u64 with a wide centre
                   window), 19 / 20 (rectified u16) and 21 / 22 (narrowed) equal tests/pixels16_ref.py exactly.

The aggregation and everything behind it consume only these verified buffers (census words, g8), unchanged kernels all: together
with the two identities, which run them end to end, this covers the path.

Shapes, the smallest that hit the kernels' corners: 70x33 (W no multiple of 64, H none of 16), 65x17 (one column spills into a second
block; W odd: rows are only 2-byte aligned), 5x9 (the window does not fit: every word 0, and still written), 131x21 as a batch of 3
(W * H odd: frame 1 starts at an odd sample), 40x24 with dmin 3."""
import numpy as np
import pytest

import census_sym_ref as CS
import confidence_ref as CR
import pixels16_ref as P
import rectify_ref as RR
from conftest import load_npz
from oracle.pyoracle import STAGE_NAMES, default_option
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SHAPES = [(70, 33, 0, 16, 1), (65, 17, 0, 8, 1), (5, 9, 0, 8, 1), (131, 21, 0, 16, 3), (40, 24, 3, 19, 1)]    # W, H, dmin, dmax, batch
IDS = [f"{s[0]}x{s[1]}_d{s[2]}-{s[3]}_b{s[4]}" for s in SHAPES]


@pytest.fixture(scope="module")
def pairs8():
    """shape -> (left, right) u8 [B][H][W], built from the tiny golden inputs (cropped; 131 columns are two crops side by side,
    the same cut in both views); shared by the tests and left unchanged"""
    a = load_npz("tiny_t70x33_d16.npz")
    b = load_npz("tiny_t40x24_d16_dmin3.npz")
    out = {}
    for shape in SHAPES:
        w, h, _, _, B = shape
        frames = []
        for k in range(B):
            if (w, h) == (40, 24):
                frames.append((b["left"], b["right"]))
            elif w <= 70:
                frames.append((a["left"][k:k + h, :w], a["right"][k:k + h, :w]))
            else:
                frames.append(tuple(np.hstack([a[v][k:k + h, :70], a[v][k + 3:k + 3 + h, 70 - (w - 70):70]]) for v in ("left", "right")))
        out[shape] = tuple(np.ascontiguousarray(np.stack([f[v] for f in frames])) for v in (0, 1))
        assert out[shape][0].shape == (B, h, w)
    return out


def options(shape, flat=False, **kw):
    """flat: p2_init <= p1, the P2 table is the constant P1 (the rank identity's option)"""
    _, _, dmin, dmax, _ = shape
    if flat:
        kw.update(p1=10, p2_init=7)
    return default_option(dmax, dmin, min_speckle_area=9, **kw)


def instance(bits, batch=1, setup=None, keep=True):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0, batch=batch)
    i.keep_stages(keep)
    if setup:
        setup(i)
    assert i.set_pixel_bits(bits)
    return i


def squeeze(a, batch):
    return a[0] if batch == 1 else a


def check_frames(i, out, want_of_frame, batch, what):
    for k in range(batch):
        want = want_of_frame(k)
        i.select_frame(k)
        got = i.read_stages()
        for n in STAGE_NAMES:
            if want[n] is not None:
                assert_same(got[n], want[n], f"{what} frame {k}:{n}")
        assert_same(out[k] if batch > 1 else out, want["final"], f"{what} frame {k}:result")


# ---- the three checks on every shape -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shift_identity_every_stage_equals_the_oracle(oracle, pairs8, shape):
    w, h, _, _, B = shape
    l8, r8 = pairs8[shape]
    opt = options(shape)                                              # adaptive P2: g8 == u8 feeds it
    i = instance(12, B)
    try:
        assert i.reset(w, h, opt)
        out = i.match(squeeze(P.widen(l8, 12), B), squeeze(P.widen(r8, 12), B))
        assert out is not None
        check_frames(i, out, lambda k: oracle.run(l8[k], r8[k], opt), B, f"shift {shape}")
        for k in range(B):
            i.select_frame(k)
            gl, gr = i.read_narrowed()
            assert_same(gl, l8[k], "g8 left")
            assert_same(gr, r8[k], "g8 right")
    finally:
        i.close()


@pytest.mark.parametrize("bits", [12, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rank_identity_every_stage_equals_the_oracle_on_the_ranks(oracle, pairs8, shape, bits):
    w, h, _, _, B = shape
    l8, r8 = pairs8[shape]
    l16, r16 = P.lut_pair(l8, r8, bits, seed=bits * 1000 + w)
    ranks = [P.rank_pair(l16[k], r16[k]) for k in range(B)]
    opt = options(shape, flat=True)
    i = instance(bits, B)
    try:
        assert i.reset(w, h, opt)
        out = i.match(squeeze(l16, B), squeeze(r16, B))
        assert out is not None
        want = [oracle.run(ranks[k][0], ranks[k][1], opt) for k in range(B)]
        check_frames(i, out, lambda k: want[k], B, f"rank {shape} {bits} bits")
        if w > 5 and h > 5:
            # the tone-mapped pair matches differently: the low bits carry census comparisons
            narrowed = oracle.run(P.narrow(l16[0], bits), P.narrow(r16[0], bits), opt)
            assert not np.array_equal(narrowed["census_l"], want[0]["census_l"])
            differs = [n for n in STAGE_NAMES if not np.array_equal(narrowed[n].view(np.uint8), want[0][n].view(np.uint8))]
            print(f"{shape} {bits} bits: the 8-bit match of g8 differs from the {bits}-bit match in {differs}")
            assert "final" in differs or "aggr" in differs
    finally:
        i.close()


@pytest.mark.parametrize("kind,cw,ch", [(0, 5, 5), (1, 7, 7), (0, 9, 7)], ids=["centre5x5", "sym7x7", "wide9x7_u64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stages_of_arbitrary_content_equal_the_restatement(shape, kind, cw, ch):
    w, h, _, _, B = shape
    bits = 12
    rng = np.random.default_rng(w * 100 + h + cw)
    left, right = (rng.integers(0, 65536, (B, h, w), dtype=np.uint16) for _ in range(2))    # 15/16 of the samples are >= 2^12
    left[:, ::2, ::3] &= 0x0FFF                                                          # ... a sixth of them brought below
    lx, ly = RR.model_maps(RR.SMALL, w, h)
    rx, ry = RR.model_maps(RR.SMALL, w, h, sign=-1.0)
    opt = options(shape)
    for rectify in (False, True):
        i = instance(bits, B, lambda i: i.set_census_kind(kind) and i.set_census_window(cw, ch))
        try:
            if rectify:
                assert i.set_rectify(lx, ly, rx, ry)
            assert i.reset(w, h, opt)
            assert i.match(squeeze(left, B), squeeze(right, B)) is not None
            for k in range(B):
                i.select_frame(k)
                src_l, src_r = (P.remap(left[k], lx, ly), P.remap(right[k], rx, ry)) if rectify else (left[k], right[k])
                what = f"{shape} kind {kind} {cw}x{ch} rectify {rectify} frame {k}"
                if rectify:
                    got_l, got_r = i.read_rectified()
                    assert got_l.dtype == np.uint16
                    assert_same(got_l, src_l, what + ": stage 19")
                    assert_same(got_r, src_r, what + ": stage 20")
                cl, cr = i.read_stage(0), i.read_stage(1)
                assert cl.dtype == (np.uint64 if (kind == 0 and (cw, ch) != (5, 5)) else np.uint32)
                assert_same(cl, P.census(src_l, kind, cw, ch), what + ": stage 0")
                assert_same(cr, P.census(src_r, kind, cw, ch), what + ": stage 1")
                gl, gr = i.read_narrowed()
                assert_same(gl, P.narrow(src_l, bits), what + ": stage 21")
                assert_same(gr, P.narrow(src_r, bits), what + ": stage 22")
        finally:
            i.close()


# ---- options, each once on 70x33 -----------------------------------------------------------------------------------------------

BASE = SHAPES[0]


def outputs(i, left, right, how="match"):
    """everything a match of kind `how` returns and leaves readable, as a dict of arrays"""
    out = {}
    if how == "confidence":
        out["result"], out["conf"] = i.match_confidence(left, right)
    elif how == "both":
        out["result"], out["right"] = i.match_both(left, right)
        out["stage28"] = i.read_stage(28)
    else:
        out["result"] = i.match(left, right)
        assert out["result"] is not None
    for n in STAGE_NAMES:
        out[n] = i.read_stage(n)
    return out


def same_outputs(got, want, what):
    assert got.keys() == want.keys()
    for n in want:
        assert_same(got[n], want[n], f"{what}:{n}")


def twin_check(pairs8, setup, bits=12, how="match", what="", opt_kw=None, calls=1, identities=("shift", "rank")):
    """Both identities against the 8-bit match of an instance set up the same way: (u8 << shift at `bits`) against u8 with the
    adaptive P2; lut[u8] against its ranks with the flat P2.  calls: matches per reset (2: the second adds to the first's S)."""
    w, h = BASE[0], BASE[1]
    l8, r8 = (a[0] for a in pairs8[BASE])
    l16, r16 = P.lut_pair(l8, r8, bits, seed=77)
    rl, rr = P.rank_pair(l16, r16)
    cases = [("shift", (l8, r8), (P.widen(l8, bits), P.widen(r8, bits)), options(BASE, **(opt_kw or {}))),
             ("rank", (rl, rr), (l16, r16), options(BASE, flat=True, **(opt_kw or {})))]
    i8, i16 = instance(8, setup=setup), instance(bits, setup=setup)
    try:
        for name, small, big, opt in cases:
            if name not in identities:
                continue
            assert i8.reset(w, h, opt) and i16.reset(w, h, opt)
            for c in range(calls):
                want, got = outputs(i8, *small, how), outputs(i16, *big, how)
                same_outputs(got, want, f"{what} {name} call {c}")
            gl, gr = i16.read_narrowed()
            assert_same(gl, P.narrow(big[0], bits), f"{what} {name}: stage 21")
            assert_same(gr, P.narrow(big[1], bits), "stage 22")
    finally:
        i8.close()
        i16.close()


@pytest.mark.parametrize("bits", [10, 12, 16])
def test_bits(pairs8, bits):
    twin_check(pairs8, None, bits=bits, what=f"{bits} bits")


@pytest.mark.parametrize("kind,cw,ch", [(1, 7, 7), (1, 9, 7), (0, 7, 7), (0, 9, 7)], ids=["sym7x7", "sym9x7", "wide7x7", "wide9x7"])
def test_census_kinds_and_windows(pairs8, kind, cw, ch):
    twin_check(pairs8, lambda i: i.set_census_kind(kind) and i.set_census_window(cw, ch), what=f"kind {kind} {cw}x{ch}")


def test_four_path_mode(pairs8):
    twin_check(pairs8, lambda i: i.set_honor_num_paths(True), what="four paths", opt_kw={"num_paths": 4})


def test_right_reference_view(pairs8):
    twin_check(pairs8, lambda i: i.set_reference_view(True), what="right view")


def test_match_both(pairs8):
    twin_check(pairs8, None, how="both", what="both views")


def test_confidence(oracle, pairs8):
    twin_check(pairs8, None, how="confidence", what="confidence")
    # ... and against the checker's costs, through the rank identity
    w, h = BASE[0], BASE[1]
    l16, r16 = P.lut_pair(*(a[0] for a in pairs8[BASE]), 12, seed=5)
    opt = options(BASE, flat=True)
    want = oracle.run(*P.rank_pair(l16, r16), opt)
    i = instance(12, keep=False)
    try:
        assert i.reset(w, h, opt)
        disp, conf = i.match_confidence(l16, r16)
        assert_same(disp, want["final"], "confidence: map")
        assert_same(conf, CR.confidence(want["aggr"], 0, False)[3], "confidence")
    finally:
        i.close()


def test_hole_filling(oracle, pairs8):
    import fill_holes_ref as FH
    twin_check(pairs8, lambda i: i.set_fill_holes(True), what="hole filling")
    w, h = BASE[0], BASE[1]
    l16, r16 = P.lut_pair(*(a[0] for a in pairs8[BASE]), 12, seed=6)
    opt = options(BASE, flat=True)
    want = oracle.run(*P.rank_pair(l16, r16), opt)
    cls, filled, final = FH.expected(want, opt, oracle)
    i = instance(12)
    try:
        assert i.set_fill_holes(True) and i.reset(w, h, opt)
        got = i.match(l16, r16)
        assert_same(i.read_fill_classes(), cls, "classes")
        assert_same(i.read_filled(), filled, "stage 9")
        assert_same(got, final, "final")
    finally:
        i.close()


def test_refinement_is_guided_by_the_narrowed_image(oracle, pairs8):
    """lut pair, flat P2: the map before the refinement is the oracle's on the ranks; the refined map must be the restatement's
    refinement of it guided by g8 -- not by the ranks, not by the u16 samples -- which is also what stages 21 / 22 hold."""
    import refine_ref as R
    import soc_project_stereo_matching_amd as S
    w, h = BASE[0], BASE[1]
    l16, r16 = P.lut_pair(*(a[0] for a in pairs8[BASE]), 12, seed=8)
    rl, rr = P.rank_pair(l16, r16)
    opt = options(BASE, flat=True)
    lam, sigma, T = S.REFINE_LAMBDA, S.REFINE_SIGMA, S.REFINE_ITERS
    tabs = R.tables(lam, sigma, T, S.load_library())
    for right_view in (False, True):
        oracle.set_reference_view(right_view)
        try:
            want = oracle.run(rl, rr, opt)
        finally:
            oracle.set_reference_view(False)
        conf = CR.confidence(want["aggr"], 0, right_view)[3]
        g8 = P.narrow(r16 if right_view else l16, 12)
        refined = R.refine(want["final"], conf, g8, tabs, False)
        assert not np.array_equal(refined.view(np.uint32), R.refine(want["final"], conf, rr if right_view else rl, tabs, False).view(np.uint32))
        i = instance(12, keep=False)
        try:
            i.set_reference_view(right_view)
            assert i.set_refine(True, lam, sigma, T, False) and i.reset(w, h, opt)
            assert_same(i.match(l16, r16), refined, f"refined map, right view {right_view}")
            assert_same(i.read_narrowed()[1 if right_view else 0], g8, "the guide's source")
        finally:
            i.close()
    # (the rank identity does not reach behind the refinement: its guide is g8, the twin's is the rank image -- the case above)
    twin_check(pairs8, lambda i: i.set_refine(True, lam, sigma, T, False), what="refinement", identities=("shift",))


def test_match_without_reset_accumulates(pairs8):
    twin_check(pairs8, None, what="no reset", calls=2)


def test_overlap_post(pairs8):
    twin_check(pairs8, lambda i: i.set_overlap_post(True), what="overlap post", calls=2)


# ---- rectification -------------------------------------------------------------------------------------------------------------

def device_u16(host, torch):
    """(buffer, pointer): the samples at a 16-byte-aligned base + 2 bytes, a canary of 16 bytes behind them"""
    raw = np.ascontiguousarray(host).view(np.uint8).ravel()
    buf = torch.full((raw.size + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[2:2 + raw.size] = torch.from_numpy(raw).cuda()
    return buf, buf.data_ptr() + 2


def test_rectification_on_device_images_and_identity_maps(pairs8):
    import torch
    w, h = BASE[0], BASE[1]
    rng = np.random.default_rng(19)
    left, right = (rng.integers(0, 65536, (h, w), dtype=np.uint16) for _ in range(2))
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    non_integer = (x + np.float32(0.3) + (x % 32) / 32, y + np.float32(0.7) - (y % 5) / 8)       # taps beyond the right and bottom border too
    for name, (mx, my) in (("non-integer", non_integer), ("identity", (x, y)), ("model", RR.model_maps(RR.RADIAL, w, h))):
        rx, ry = np.ascontiguousarray(mx[:, ::-1]), np.ascontiguousarray(my[::-1, :])
        i = instance(12)
        try:
            assert i.set_rectify(mx, my, rx, ry) and i.reset(w, h, options(BASE))
            want_l, want_r = P.remap(left, mx, my), P.remap(right, rx, ry)
            if name == "identity":
                assert np.array_equal(want_l, left)
            (bl, pl), (br, pr) = device_u16(left, torch), device_u16(right, torch)
            (bol, pol), (bor, por) = device_u16(np.zeros_like(left), torch), device_u16(np.zeros_like(right), torch)
            torch.cuda.synchronize()
            assert i.rectify(pl, pr, pol, por) and i.synchronize()
            for buf, want, side in ((bol, want_l, "left"), (bor, want_r, "right")):
                got = buf.cpu().numpy()
                assert np.all(got[:2] == 0xA5) and np.all(got[2 + 2 * w * h:] == 0xA5), f"{name} {side}: wrote outside the image"
                assert_same(got[2:2 + 2 * w * h].view(np.uint16).reshape(h, w), want, f"{name}: sgm_rectify {side}")
            assert not i.rectify(pl + 1, pr, pol, por)                                         # an odd address is refused
            assert i.match(left, right) is not None
            got_l, got_r = i.read_rectified()
            assert_same(got_l, want_l, f"{name}: stage 19")
            assert_same(got_r, want_r, f"{name}: stage 20")
            assert_same(i.read_stage(0), P.census_centre(want_l), f"{name}: the census saw the rectified image")
        finally:
            i.close()


# ---- device images, instance reuse, the interface ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_device_images_two_bytes_past_an_aligned_base(pairs8, shape):
    """W odd, and (batch) W * H odd: rows and frames start at every 2-byte phase of 16 bytes.  The device-pointer match of images
    at base + 2 must equal the host-pointer match, stage by stage, and an odd address must be refused."""
    import torch
    w, h, _, _, B = shape
    l16, r16 = P.lut_pair(*pairs8[shape], 12, seed=3)
    opt = options(shape)
    a, b = instance(12, B), instance(12, B)
    try:
        assert a.reset(w, h, opt) and b.reset(w, h, opt)
        want = a.match(squeeze(l16, B), squeeze(r16, B))
        (bl, pl), (br, pr) = device_u16(l16, torch), device_u16(r16, torch)
        d_out = torch.zeros((B, h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert not b.match_device(pl + 1, pr, d_out.data_ptr()) and not b.match_device(pl, pr - 1, d_out.data_ptr())
        assert b.match_device(pl, pr, d_out.data_ptr()) and b.synchronize()
        assert_same(squeeze(d_out.cpu().numpy(), B), want, "device images: result")
        for k in range(B):
            a.select_frame(k)
            b.select_frame(k)
            for n in STAGE_NAMES[:-1]:                                 # (the final map of a device-pointer match is in the caller's buffer)
                assert_same(b.read_stage(n), a.read_stage(n), f"device images frame {k}:{n}")
        assert np.all(bl.cpu().numpy()[2 + 2 * l16.size:] == 0xA5)                             # the images are only read
    finally:
        a.close()
        b.close()


def test_one_instance_through_8_12_8_bits(oracle, pairs8):
    w, h = BASE[0], BASE[1]
    l8, r8 = (a[0] for a in pairs8[BASE])
    l16, r16 = P.lut_pair(l8, r8, 12, seed=4)
    opt = options(BASE)
    i, fresh = instance(8), instance(8)
    try:
        assert i.reset(w, h, opt) and fresh.reset(w, h, opt)
        want = outputs(fresh, l8, r8)
        same_outputs(outputs(i, l8, r8), want, "8 bits, first")
        with pytest.raises(TypeError):
            i.match(l16, r16)                                          # uint16 arrays do not fit an 8-bit instance
        assert i.set_pixel_bits(12)
        assert i.match(l8, r8) is None                                 # a change of bits takes effect at the next initialize / reset
        assert i.reset(w, h, opt)
        with pytest.raises(TypeError):
            i.match(l8, r8)
        twelve = outputs(i, l16, r16)                                  # the lut keeps the order: the same words, another grey image
        assert_same(twelve["census_l"], want["census_l"], "12 bits: census")
        assert_same(i.read_narrowed()[0], P.narrow(l16, 12), "12 bits: stage 21")
        assert not np.array_equal(P.narrow(l16, 12), l8) and not np.array_equal(twelve["aggr"], want["aggr"])
        assert i.set_pixel_bits(8) and i.reset(w, h, opt)
        same_outputs(outputs(i, l8, r8), want, "8 bits again")
        assert i.lib.sgm_read_stage(i.handle, 21, l8.copy().ctypes.data, l8.nbytes) == 0
        assert_same(want["result"], oracle.run(l8, r8, opt)["final"], "8 bits against the oracle")
    finally:
        i.close()
        fresh.close()


def test_setter_refusals_and_the_default_instance(oracle, pairs8):
    import soc_project_stereo_matching_amd as S
    w, h = BASE[0], BASE[1]
    l8, r8 = (a[0] for a in pairs8[BASE])
    opt = options(BASE)
    i = S.SGMInstance(0)
    try:
        for bad in (7, 17, -1):
            assert not i.set_pixel_bits(bad)
        assert i.set_pixel_bits(12) and i.set_rows(4, 12) and not i.reset(w, h, opt)        # row tiles are refused
        assert i.set_rows(0, 0) and i.reset(w, h, opt)
        planes, depth = np.zeros((6, h, w), np.uint8), np.zeros((h, w), np.float32)
        assert not i.match_planes(planes, 700.0, 160.0, 0.0, depth)                           # byte planes by protocol
        assert i.match(P.widen(l8, 12), P.widen(r8, 12)) is not None and i.fused_sweep_rows() == 0
    finally:
        i.close()
    want = oracle.run(l8, r8, opt)["final"]
    g = S.SGM()
    g.shutdown()
    try:
        assert not g.set_pixel_bits(17) and g.set_pixel_bits(16)
        assert g.reset(w, h, opt)
        assert_same(g.match(P.widen(l8, 16), P.widen(r8, 16)), want, "default instance")
        g.shutdown()                                                   # a new default instance: the setting stays
        assert_same(g.compute(P.widen(l8, 16), P.widen(r8, 16), opt), want, "default instance, re-created")
        assert_same(g.read_stage(S.STAGE_NARROW_LEFT), l8, "stage 21 of the default instance")
    finally:
        g.set_pixel_bits(8)
        g.shutdown()
    assert g.reset(w, h, opt)
    assert_same(g.match(l8, r8), want, "8 bits again")
    g.shutdown()
