"""Matching at 1/f scale (extension; include/sgm_mi355x.h, sgm_scale_spec) on an MI355X against the numpy restatement
tests/scaled_ref.py.  Tolerance 0 everywhere: the downscale and the re-search are integer arithmetic, the sub-pixel term is three
IEEE float32 operations, so arrays are compared byte for byte, and every output buffer carries canary bytes (0xA5) behind its end.

Shapes, the smallest that hit the kernels' corners: 64x16 (exact multiples of the factor and of the 64-wide workgroup), 67x19 and
70x23 (remainders on both axes, a second workgroup column of 3 / 6 pixels), f x f (one output sample), 5x5 (the 9x9 window is larger
than the frame: most terms cost 24).

The composed call against its whole contract (the table in DESIGN.md, "Matching at 1/f scale"): the case lists and their references
live in tests/scaled_cases.py, whose quotas tests/test_scaled_cpu.py evaluates without a GPU and every test here asserts again on
`want` before it compares.  Option by option (test_composed_options), one live instance through changing shapes, factors, radii,
bits and batches, also under the debug allocation mode (test_one_live_instance*), queued calls with the post pass on a stream or on
compute units of its own (test_queued_*), the re-search kernel alone on planted inputs (test_upscale_on_planted_cases) and the
ends of the spec, 65535 wide and 65535 tall (test_*_at_the_ends_of_the_spec)."""
import ctypes as C

import numpy as np
import pytest

import census_sym_ref as CS
import instance_steps as IR
import pixels16_ref as P
import scaled_cases as SC
import scaled_ref as SR
from oracle.pyoracle import default_option
from scaled_cases import planted, scene                              # (tests/test_gpu_guard_bands.py imports them from here)

pytestmark = pytest.mark.gpu

CANARY = 64


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.tobytes() != want.tobytes():
        word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        bad = np.flatnonzero(got.view(word).ravel() != want.view(word).ravel())
        k = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {np.unravel_index(k, got.shape)}: "
                             f"got {got.ravel()[k]!r}, want {want.ravel()[k]!r}")


def to_device(a, offset_elems=0):
    """a device copy of a numpy array (u16 travels as int16), optionally `offset_elems` elements off an aligned allocation"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    src = torch.from_numpy(flat.view(np.int16) if flat.dtype == np.uint16 else flat.view(np.int32) if flat.dtype == np.uint32 else flat)
    hold = torch.empty(flat.size + 64, dtype=src.dtype, device="cuda")
    t = hold[offset_elems:offset_elems + flat.size]
    t.copy_(src)
    return t


class Out:
    """an output buffer of n elements of a numpy dtype, 0xA5 everywhere, with CANARY bytes behind its end (and, `offset_elems` elements
    off its aligned allocation, that many in front of it)"""
    def __init__(self, n, dtype, offset_elems=0):
        import torch
        self.n, self.dtype = n, np.dtype(dtype)
        self.lo = offset_elems * self.dtype.itemsize
        self.t = torch.full((self.lo + n * self.dtype.itemsize + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + self.lo

    def read(self, shape, what):
        raw = self.t.cpu().numpy()
        end = self.lo + self.n * self.dtype.itemsize
        assert (raw[end:] == 0xA5).all(), f"{what}: bytes behind the end of the output were written"
        assert (raw[:self.lo] == 0xA5).all(), f"{what}: bytes in front of the output were written"
        return raw[self.lo:end].copy().view(self.dtype).reshape(shape)


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    yield i
    i.close()


def spec_of(W, H, f, frames=1, bits=8, radius=3, penalty=1, d_lo=0, d_hi=65535):
    import soc_project_stereo_matching_amd as S
    return S.scale_spec(W, H, f, frames=frames, bits=bits, radius=radius, penalty=penalty, d_lo=d_lo, d_hi=d_hi)


# ---- downscale --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 12, 16])
@pytest.mark.parametrize("f", [2, 4])
def test_downscale(inst, f, bits):
    import soc_project_stereo_matching_amd as S
    rng = np.random.default_rng(100 * f + bits)
    dt = np.uint16 if bits > 8 else np.uint8
    for (W, H) in ((64, 16), (67, 19), (f, f)):
        sp = spec_of(W, H, f, frames=3, bits=bits)
        assert S.scaled_shape(sp) == (W // f, H // f)
        for content in ("random", "maximum"):
            img = rng.integers(0, 1 << bits, (3, H, W)).astype(dt) if content == "random" else np.full((3, H, W), (1 << bits) - 1, dt)
            want = SR.downscale(img, f)
            for off in (0, 1):                                       # an aligned pointer, and one element off an aligned allocation
                what = f"{W}x{H} f={f} bits={bits} {content} offset {off}"
                src = to_device(img, off)
                assert src.data_ptr() % 16 == off * dt().itemsize
                out = Out(want.size, dt)
                assert inst.downscale(sp, src.data_ptr(), out.ptr()), what
                assert inst.synchronize(), what
                same(out.read(want.shape, what), want, what)
                if content == "maximum":
                    assert (want == (1 << bits) - 1).all()


# ---- upscale on planted inputs -----------------------------------------------------------------------------------------------------

def run_upscale(inst, sp, arrays, right, what, offset=0, want=None):
    """offset: every array and the output `offset` elements off an aligned allocation; want: the reference where the caller has it"""
    small, g_small, g_full, c_ref, c_oth = arrays
    dev = [to_device(a, offset) for a in arrays]
    if offset:
        assert all(t.data_ptr() % 16 == offset * t.element_size() for t in dev)
    planes = (dev[3].data_ptr(), dev[4].data_ptr()) if sp.radius >= 0 else (None, None)
    out = Out(g_full.size, np.float32, offset)
    assert inst.upscale_disparity(sp, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), planes[0], planes[1], right, out.ptr()), what
    assert inst.synchronize(), what
    got = out.read(g_full.shape, what)
    if want is None:
        want = SR.upscale_batch(small, g_small, g_full, c_ref, c_oth, sp.factor, sp.radius, sp.penalty, sp.d_lo, sp.d_hi, right)
    same(got, want, what)
    return got


@pytest.mark.parametrize("W,H,f,bits", [(67, 19, 2, 8), (70, 23, 4, 12), (5, 5, 2, 8)], ids=["67x19_f2", "70x23_f4_12bit", "5x5_f2"])
def test_upscale_on_planted_inputs(inst, W, H, f, bits):
    rng = np.random.default_rng(W * 1000 + H)
    d_lo, d_hi = 3, 3 + (W * 2) // 3                               # the map's values run from -f to d_hi + 2 f: clipped at both ends
    seen_sub = seen_prior = False
    # radius x view x hole share x penalty, fully crossed: every penalty meets finite priors with every radius and both views, on
    # the SAME planted arrays, so that the penalty is the only thing that differs between the three maps of a set
    for radius in (-1, 0, 3, 4):
        for right in (False, True):
            for inf_share in (0, 0.3, 1):
                arrays = planted(rng, W, H, f, 2, bits, inf_share, d_hi + 2 * f)
                maps = {}
                for penalty in (0, 1, 16):
                    sp = spec_of(W, H, f, frames=2, bits=bits, radius=radius, penalty=penalty, d_lo=d_lo, d_hi=d_hi)
                    what = f"{W}x{H} f={f} r={radius} pen={penalty} right={right} inf={inf_share}"
                    got = maps[penalty] = run_upscale(inst, sp, arrays, right, what)
                    if inf_share == 1:
                        assert np.isposinf(got).all(), what
                        continue
                    fin = np.isfinite(got)
                    assert fin.any(), what
                    if radius >= 0:                                # only the re-search rounds to integers and clips
                        seen_sub |= bool((got[fin] != np.rint(got[fin])).any())
                        seen_prior |= bool((got[fin] > d_hi).any() or (got[fin] < d_lo).any())   # no candidate admitted: the prior
                if radius >= 0 and inf_share != 1 and W > 9:
                    # the pull toward the prior decides pixels: 16 half bits per window pixel and step outweigh random words' costs
                    # (not asserted in the 5x5 frame, where few candidates are admitted and most terms are the constant 24)
                    assert not np.array_equal(maps[0].view(np.uint32), maps[16].view(np.uint32)), (radius, right, inf_share)
    assert seen_sub and seen_prior                                 # the content reached the sub-pixel term and the clipped ends


def test_upscale_with_one_admitted_disparity(inst):
    """d_lo == d_hi: no neighbour is admitted, so no sub-pixel term applies and every searched pixel is exactly d_lo"""
    W, H, f = 67, 19, 2
    rng = np.random.default_rng(7)
    sp = spec_of(W, H, f, frames=2, radius=3, penalty=1, d_lo=9, d_hi=9)
    arrays = planted(rng, W, H, f, 2, 8, 0.3, 20)
    got = run_upscale(inst, sp, arrays, False, "d_lo == d_hi")
    pr = SR.upscale_batch(*arrays[:3], None, None, f, -1, 0, 0, 0, False)
    near = np.isfinite(pr) & (np.abs(np.rint(pr) - 9) <= f)
    assert near.any() and (got[near] == 9).all()
    same(got[~near], pr[~near], "pixels without an admitted candidate keep the prior")


# ---- the composed match ------------------------------------------------------------------------------------------------------------

def small_finals(oracle, ls, rs, opt, bits, symmetric, right_view, times=1):
    """the oracle's final map of one small pair; times = 2: of the second of two matches without Reset (the sums add up, Q14)"""
    if not symmetric and bits == 8:
        oracle.set_reference_view(right_view)
        try:
            oracle.clear_census()
            assert oracle.reset(ls.shape[1], ls.shape[0], opt)
            for _ in range(times):
                final = oracle.match(ls, rs)
        finally:
            oracle.set_reference_view(False)
        return final
    words = (P.census_sym(ls, 7, 7), P.census_sym(rs, 7, 7))
    l8, r8 = (P.narrow(ls, bits), P.narrow(rs, bits)) if bits > 8 else (ls, rs)
    st = CS.pipeline(oracle, l8, r8, opt, 7, 7, right_view=right_view, words=words)
    if times == 2:
        st = CS.pipeline(oracle, l8, r8, opt, 7, 7, right_view=right_view, words=words, S_prev=st["aggr"])
    return st["final"]


def full_words(oracle, img, bits, symmetric):
    if symmetric:
        return P.census_sym(img, 7, 7)
    return oracle.census(img) if bits == 8 else P.census_centre(img)


CASES = [
    # W, H, f, small D, batch, bits, symmetric, right view
    (96, 40, 2, 16, 2, 8, False, False),
    (128, 48, 4, 16, 1, 8, False, False),
    (96, 40, 2, 16, 1, 12, True, False),
    (96, 40, 2, 16, 1, 8, False, True),
]


@pytest.mark.parametrize("W,H,f,D,B,bits,symmetric,right_view", CASES,
                         ids=["96x40_f2_batch2", "128x48_f4", "12bit_symmetric7x7", "right_view"])
def test_composed_match(oracle, W, H, f, D, B, bits, symmetric, right_view):
    import soc_project_stereo_matching_amd as S
    w, h = W // f, H // f
    opt = default_option(D, 0, min_speckle_area=9)
    left, right = scene(W, H, f * 12, B, bits, 4242 + W)
    ls, rs = SR.downscale(left, f), SR.downscale(right, f)
    small = np.stack([small_finals(oracle, ls[k], rs[k], opt, bits, symmetric, right_view) for k in range(B)])
    words_l = np.stack([full_words(oracle, left[k], bits, symmetric) for k in range(B)])
    words_r = np.stack([full_words(oracle, right[k], bits, symmetric) for k in range(B)])
    guide, guide_small = (right, rs) if right_view else (left, ls)
    c_ref, c_oth = (words_r, words_l) if right_view else (words_l, words_r)
    want = SR.upscale_batch(small, guide_small, guide, c_ref, c_oth, f, S.sgm.SCALE_DEFAULT_RADIUS, S.sgm.SCALE_DEFAULT_PENALTY, 0,
                            f * D - 1, right_view)
    assert np.isfinite(want).mean() > 0.3                           # the pair matches: the comparison is not one of +INF maps

    def fresh():
        i = S.SGMInstance(0, batch=B)
        if symmetric:
            assert i.set_census_kind(S.sgm.CENSUS_SYMMETRIC) and i.set_census_window(7, 7)
        i.set_reference_view(right_view)
        assert i.set_pixel_bits(bits)
        assert i.initialize(w, h, opt)
        return i

    sp = spec_of(W, H, f, frames=B, bits=bits)
    squeeze = (lambda a: a[0]) if B == 1 else (lambda a: a)
    i = fresh()
    try:
        # the host form
        got = i.match_scaled(sp, squeeze(left), squeeze(right))
        assert got is not None
        same(got.reshape(want.shape), want, "host form")
        for k in range(B):                                           # stage 8 holds the small map
            i.select_frame(k)
            same(i.read_stage(8), small[k], f"stage 8 of frame {k}")
        # the device form, on the same instance after a Reset (without one the small match would add to the sums, Q14)
        assert i.reset(w, h, opt)
        d_l, d_r = to_device(left), to_device(right)
        out = Out(want.size, np.float32)
        assert i.match_scaled_device(sp, d_l.data_ptr(), d_r.data_ptr(), out.ptr())
        assert i.synchronize()
        same(out.read(want.shape, "device form"), want, "device form")
        # afterwards a plain match on the same instance returns what a fresh instance returns after one ordinary match
        again = i.match(squeeze(ls), squeeze(rs))
        j = fresh()
        try:
            assert j.match(squeeze(ls), squeeze(rs)) is not None
            twin = j.match(squeeze(ls), squeeze(rs))
        finally:
            j.close()
        same(again, twin, "a plain match after the scaled one")
        second = np.stack([small_finals(oracle, ls[k], rs[k], opt, bits, symmetric, right_view, times=2) for k in range(B)])
        same(again.reshape(second.shape), second, "... and the oracle's second match without Reset")
    finally:
        i.close()


def test_composed_refusals(oracle):
    import soc_project_stereo_matching_amd as S
    W, H, f = 96, 40, 2
    left, right = scene(W, H, 24, 1, 8, 1)
    opt = default_option(16)
    i = S.SGMInstance(0)
    try:
        sp = spec_of(W, H, f)
        assert i.match_scaled(sp, left[0], right[0]) is None          # not initialised
        assert i.initialize(W // f, H // f, opt)
        assert i.match_scaled(sp, left[0], right[0]) is not None
        assert i.match_scaled(spec_of(W, H, 4), left[0], right[0]) is None        # the instance is not at 24x10
        assert i.match_scaled(spec_of(W, H, f, radius=5), left[0], right[0]) is None
        assert i.match_scaled(spec_of(W, H, f, penalty=17), left[0], right[0]) is None
        assert S.scaled_shape(spec_of(3, 40, 4)) is None and S.scaled_shape(spec_of(96, 40, 3)) is None
        assert i.set_census_window(9, 7) and i.initialize(W // f, H // f, opt)    # a wide CENTRE window: u64 words
        assert i.match_scaled(sp, left[0], right[0]) is None
        assert i.match_scaled(spec_of(W, H, f, radius=-1), left[0], right[0]) is not None     # ... but the guided upscale alone runs
    finally:
        i.close()


# ---- the re-search kernel alone: the cases of tests/scaled_cases.py -----------------------------------------------------------------

def planted_spec(c):
    return spec_of(c["W"], c["H"], c["f"], frames=c["frames"], bits=c["bits"], radius=c["radius"], penalty=c["penalty"], d_lo=c["d_lo"],
                   d_hi=c["d_hi"])


@pytest.mark.parametrize("c", SC.PLANTED, ids=[c["name"] for c in SC.PLANTED])
def test_upscale_on_planted_cases(inst, c):
    """radii 1 and 2 with both factors and views (sgm_upscale_k<F, 1> and <F, 2>), three workgroup columns with a last one 2 pixels
    wide, one low-resolution row, frame offsets that are no multiple of four elements, every pointer one element off an aligned
    allocation, small-map values at the ends of float32 and of the prior's clamp, d_lo = d_hi at 0 and at 65535"""
    r = SC.planted_case(c)
    SC.planted_quotas(c, r)
    got = run_upscale(inst, planted_spec(c), r["arrays"], c["right"], c["name"], offset=c["offset"], want=r["want"])
    if c["values"] == "extremes":
        assert np.isposinf(got).any() and np.isneginf(got).any() and not np.isnan(got).any()


@pytest.mark.parametrize("c", SC.PLANTED_ENDS, ids=[c["name"] for c in SC.PLANTED_ENDS])
def test_upscale_at_the_ends_of_the_spec(inst, c):
    """65535 wide (1024 workgroup columns, the last 63 pixels wide) and 65535 tall (16384 workgroup rows, the last 3 rows high)"""
    r = SC.planted_case(c)
    SC.planted_quotas(c, r)
    run_upscale(inst, planted_spec(c), r["arrays"], c["right"], c["name"], want=r["want"])


# ---- the composed match against its whole contract ----------------------------------------------------------------------------------

def configure(i, c):
    """every option of the case on the instance, and a Reset at its small shape"""
    st, opt = SC.step_of(c), SC.option_of(c)
    IR.apply(i, st)
    assert i.reset(st["w"], st["h"], opt), c["name"]
    return st, opt


def squeeze(a):
    return a[0] if len(a) == 1 else a


def scaled_call(i, c, left, right, device, what):
    """one composed call, host form or device form, into a buffer with canary bytes behind it -> the map [B][H][W]"""
    st = SC.step_of(c)
    sp = spec_of(c["W"], c["H"], c["f"], frames=c["B"], bits=st["bits"], radius=c["radius"])
    shape = (c["B"], c["H"], c["W"])
    n = int(np.prod(shape))
    if device:
        d_l, d_r = to_device(left), to_device(right)
        out = Out(n, np.float32)
        assert i.match_scaled_device(sp, d_l.data_ptr(), d_r.data_ptr(), out.ptr()), what
        assert i.synchronize(), what
        return out.read(shape, what)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    raw = np.full(n * 4 + CANARY, 0xA5, np.uint8)
    assert i.lib.sgm_match_scaled(i.handle, C.byref(sp), left.ctypes.data, right.ctypes.data, raw.ctypes.data), what
    assert (raw[n * 4:] == 0xA5).all(), f"{what}: bytes behind the end of the host's output were written"
    return raw[:n * 4].copy().view(np.float32).reshape(shape)


def check_small(i, c, r, what):
    """stage 8 is the small final map; with keep_stages the stages the instance kept are the small match's"""
    for k in range(c["B"]):
        i.select_frame(k)
        same(i.read_stage(8), r["small"][k], f"{what}: stage 8 of frame {k}")
        if r["st"]["keep"]:
            for name in ("disp_l", "after_lr", "after_speckle", "aggr"):
                same(i.read_stage(name), r["stages"][k][name], f"{what}: kept stage {name} of frame {k}")


def composed_both_forms(oracle, c):
    """the host form and the device form of ONE instance, a Reset between them; with q14 each form is two calls without a Reset"""
    import soc_project_stereo_matching_amd as S
    assert (S.sgm.SCALE_DEFAULT_RADIUS, S.sgm.SCALE_DEFAULT_PENALTY) == (SC.RADIUS, SC.PENALTY)
    r = SC.composed(oracle, c)
    print(c["name"], SC.composed_quotas(c, r))
    i = S.SGMInstance(0)
    try:
        for device in (False, True):
            what = f"{c['name']} {'device' if device else 'host'} form"
            configure(i, c)
            if "first" in r:
                same(scaled_call(i, c, *r["first"], device, what), r["first_want"], what + ", first call")
            same(scaled_call(i, c, r["left"], r["right"], device, what), r["want"], what)
            check_small(i, c, r, what)
    finally:
        i.close()


@pytest.mark.parametrize("c", SC.COMPOSED, ids=[c["name"] for c in SC.COMPOSED])
def test_composed_options(oracle, c):
    composed_both_forms(oracle, c)


@pytest.mark.parametrize("c", SC.ENDS, ids=[c["name"] for c in SC.ENDS])
def test_composed_at_the_ends_of_the_spec(oracle, c):
    composed_both_forms(oracle, c)


# ---- one live instance ----------------------------------------------------------------------------------------------------------------

_PLAIN = {}


def walk(oracle, i):
    """ONE instance through SC.WALK: the retained buffers of the scaled match (small views, census planes, narrowed guides, the host
    form's full-resolution images and map) only grow, so every step but the largest runs in buffers sized for another.  After every
    step the comparison with that step computed alone, host form and device form by turns; then a plain match of another small
    pair WITHOUT a Reset, whose sums add to the scaled call's (Q14): what it would have returned behind an ordinary match"""
    names = [c["name"] for c in SC.WALK]
    for k, c in enumerate(SC.WALK):
        what = f"step {k} ({c['name']})"
        r = SC.composed(oracle, c)
        configure(i, c)
        same(scaled_call(i, c, r["left"], r["right"], k % 2 == 1, what), r["want"], what)
        check_small(i, c, r, what)
        pl, pr = SC.small_pair(oracle, c, 900 + names.index(c["name"]))   # (a step that comes twice matches the same pair twice)
        if c["name"] not in _PLAIN:
            _PLAIN[c["name"]] = SC.plain(oracle, c, pl, pr, [(r["ls"], r["rs"])])
        again = i.match(squeeze(pl), squeeze(pr))
        assert again is not None, what
        same(again.reshape(_PLAIN[c["name"]].shape), _PLAIN[c["name"]], what + ": a plain match behind it")


def test_one_live_instance(oracle):
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    try:
        walk(oracle, i)
    finally:
        i.close()


def test_one_live_instance_under_guard(oracle, monkeypatch):
    """the same walk with a poisoned megabyte on either side of every device buffer the library allocates and the poison 0x5A in
    every fresh payload: no band is damaged, and no result depends on bytes nobody wrote"""
    import soc_project_stereo_matching_amd as S
    from test_gpu_guard_bands import G, Guard
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(G))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    with Guard(0x5A).instances(S.SGMInstance(0), what="the walk of the scaled match") as i:
        walk(oracle, i)


# ---- streams --------------------------------------------------------------------------------------------------------------------------

STREAM_MODES = {
    "one_stream": lambda i: i.set_overlap_post(False),
    "overlap_post": lambda i: i.set_overlap_post(True),
    "post_on_its_own_cus": lambda i: i.set_cu_split("post=0:4,main=4:28"),
}


@pytest.mark.parametrize("mode", list(STREAM_MODES))
def test_queued_scaled_calls_and_a_plain_match_behind_them(oracle, mode):
    """two device-form calls on different inputs into different outputs and a plain device match of a small pair, queued without a
    synchronize between them (and without a Reset: the small sums add, Q14); one synchronize, three results.  The second call's
    downscale and small match rewrite what the first call's upscale reads, and with the post pass on a stream of its own the
    upscale has to wait for it."""
    import soc_project_stereo_matching_amd as S
    a, b = SC.STREAMS
    ra = SC.composed(oracle, a)
    rb = SC.composed(oracle, b, earlier=[(ra["ls"], ra["rs"])])
    pl, pr = SC.small_pair(oracle, a, SC.STREAM_SMALL_SEED)
    want_c = SC.plain(oracle, a, pl, pr, [(ra["ls"], ra["rs"]), (rb["ls"], rb["rs"])])
    sp = spec_of(a["W"], a["H"], a["f"])
    i = S.SGMInstance(0)
    try:
        assert STREAM_MODES[mode](i)
        configure(i, a)
        dev = [to_device(x) for x in (ra["left"], ra["right"], rb["left"], rb["right"], pl, pr)]
        out_a, out_b, out_c = Out(ra["want"].size, np.float32), Out(rb["want"].size, np.float32), Out(want_c.size, np.float32)
        assert i.match_scaled_device(sp, dev[0].data_ptr(), dev[1].data_ptr(), out_a.ptr())
        assert i.match_scaled_device(sp, dev[2].data_ptr(), dev[3].data_ptr(), out_b.ptr())
        assert i.match_device(dev[4].data_ptr(), dev[5].data_ptr(), out_c.ptr())
        assert i.synchronize()
        same(out_a.read(ra["want"].shape, "first"), ra["want"], f"{mode}: the first queued call")
        same(out_b.read(rb["want"].shape, "second"), rb["want"], f"{mode}: the second queued call")
        same(out_c.read(want_c.shape, "plain"), want_c, f"{mode}: the plain match behind them")
    finally:
        i.close()


@pytest.mark.parametrize("mode", list(STREAM_MODES))
def test_scaled_call_behind_a_pending_async_match(oracle, mode):
    """sgm_match_async is still pending (its map not handed over) when sgm_match_scaled is called: the scaled call hands the pending
    result over first, and its own small match adds to that match's sums"""
    import soc_project_stereo_matching_amd as S
    a, b = SC.STREAMS
    pl, pr = SC.small_pair(oracle, a, SC.STREAM_SMALL_SEED)
    want_p = SC.plain(oracle, a, pl, pr, [])
    rb = SC.composed(oracle, b, earlier=[(pl, pr)])
    i = S.SGMInstance(0)
    try:
        assert STREAM_MODES[mode](i)
        configure(i, a)
        l, r = np.ascontiguousarray(pl[0]), np.ascontiguousarray(pr[0])
        pending = np.full(l.shape, -7, np.float32)
        assert i.match_async(l, r, pending)
        same(scaled_call(i, b, rb["left"], rb["right"], False, mode), rb["want"], f"{mode}: the scaled call")
        assert i.match_wait()
        same(pending[None], want_p, f"{mode}: the pending match")
    finally:
        i.close()
