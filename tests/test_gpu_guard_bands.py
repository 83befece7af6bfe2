"""Guard bands and poisoned buffers: where the kernels touch memory -- needs an MI355X.

Every scenario below runs with the debug allocation mode on (SGM_DEBUG_GUARD = 1 MiB, SGM_DEBUG_POISON; csrc/sgm_guard.h,
DESIGN.md "Guard bands"): each device buffer the library allocates carries a poisoned megabyte on either side and is itself full of
the poison before anybody writes it.  Two things are asserted, both with tolerance 0:

  * the outputs equal what the feature's own test compares them with (the CPU oracle, census_sym_ref, fill_holes_ref,
    confidence_ref, refine_ref, rectify_ref, pixels16_ref, scaled_ref, temporal_ref, cloud_ref) -- a result that differs under
    poison depends on bytes nobody wrote;
  * sgm_debug_guard_check() finds every band intact, with the instance alive and again after it is closed (the violations a free
    found are sticky) -- a changed band is a write outside a payload.

Both poisons run, 0xFF and 0x5A: as words a NaN and a large finite float, 255 and 90 as costs, -1 and a large count as labels or
progress words.  A stray write of the very byte a band holds, or a stale read that happens to be harmless for one value, shows
under the other.  Caller-owned device memory gets the same treatment from this module (Guard.buf): 64 KiB fences of the poison on
either side of exactly the bytes the entry point owns.

The helpers of the feature tests are imported, not restated.  tests/test_guard_cpu.py has the registry's own arithmetic."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_ref as CLR
import limits as LM
import pixels16_ref as P
import rectify_ref as RR
import scaled_ref as SR
import temporal_cases as TC
import temporal_ref as TR
from oracle.pyoracle import Oracle, default_option
from test_gpu_pixels16 import pairs8  # noqa: F401  (a fixture: the 8-bit pairs of that module's shapes)
from test_gpu_instance_reuse import LADDER, SYMMETRIC, _tile, assert_same, drive, expected, frames_of, ladder, new_instance, option_of, step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 1 << 20                      # past the longest look-behind the design admits (the census slack, ~260 KB) and any plane row here
FENCE = 64 << 10
POISONS = (0xFF, 0x5A)


class Fenced:
    """nbytes of caller-owned device memory, `skew` bytes off an aligned base, FENCE bytes of the poison on either side, the region
    itself poisoned too"""
    def __init__(self, poison, nbytes, skew=0):
        import torch
        self.poison, self.n, self.lo = poison, int(nbytes), FENCE + skew
        self.t = torch.full((self.lo + self.n + FENCE,), poison, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.lo
        torch.cuda.synchronize()
        assert (self.t.data_ptr() % 256 == 0) and self.ptr % 256 == skew

    def put(self, a):
        import torch
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        assert raw.size == self.n, (raw.size, self.n)
        self.t[self.lo:self.lo + self.n].copy_(torch.from_numpy(raw.copy()))
        torch.cuda.synchronize()                              # the library's streams do not wait for torch's
        return self

    def get(self, dtype, shape=(-1,)):
        return self.t[self.lo:self.lo + self.n].cpu().numpy().view(dtype).reshape(shape).copy()

    def check(self, what=""):
        raw = self.t.cpu().numpy()
        for side, part in (("front", raw[:self.lo]), ("back", raw[self.lo + self.n:])):
            bad = np.flatnonzero(part != self.poison)
            if bad.size:
                raise AssertionError(f"{what}: the {side} fence of a caller's buffer of {self.n} bytes was written, "
                                     f"{bad.size} bytes, offsets {bad[0]}..{bad[-1]} of that fence")


class Guard:
    def __init__(self, poison):
        self.poison, self.fences = poison, []

    def buf(self, data, skew=0):
        """a fenced buffer: data is a byte count (an output: poison inside) or an array (an input: its bytes inside)"""
        if isinstance(data, (int, np.integer)):
            f = Fenced(self.poison, data, skew)
        else:
            f = Fenced(self.poison, np.ascontiguousarray(data).nbytes, skew).put(data)
        self.fences.append(f)
        return f

    def check_fences(self, what=""):
        import torch
        torch.cuda.synchronize()
        for f in self.fences:
            f.check(what)
        self.fences = []

    @staticmethod
    def verify(what, live_wanted=True):
        import torch
        import soc_project_stereo_matching_amd as S
        torch.cuda.synchronize()
        bad, live, size = S.debug_guard_check()
        assert bad == 0, f"{what}: {bad} guard band(s) violated (the lines on stderr say where)"
        if live_wanted:
            assert live > 0 and size > 0, f"{what}: nothing under guard -- the mode is off"
        else:
            assert live == 0, f"{what}: {live} guarded buffers outlive their instances"

    @contextlib.contextmanager
    def instances(self, *made, what=""):
        """the instances of one scenario: checked alive, closed, checked again -- whatever the body did"""
        try:
            yield made[0] if len(made) == 1 else made
            assert all(i.synchronize() for i in made), what
            self.check_fences(what)
            self.verify(what + " (instance alive)")
        finally:
            for i in made:
                i.close()
        self.verify(what + " (instance closed)", live_wanted=False)


@pytest.fixture(params=POISONS, ids=["poisonFF", "poison5A"])
def guard(request, monkeypatch):
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)                 # nothing left over from whoever ran before
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(G))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(request.param))
    g = Guard(request.param)
    yield g
    g.check_fences("teardown")
    g.verify("teardown", live_wanted=False)


def fresh(monkeypatch, env=None, batch=1):
    import soc_project_stereo_matching_amd as S
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))                         # read at sgm_create / at the launch
    return S.SGMInstance(0, batch=batch)


def drive_fresh(guard, oracle, monkeypatch, env, steps, what, seed):
    """every step on an instance of its own: whatever it allocates is junk at exactly that shape"""
    for k, st in enumerate(steps):
        tag = f"{what} {st['w']}x{st['h']} d{st['d']} dmin{st['dmin']} b{st['batch']}"
        with guard.instances(new_instance(monkeypatch, env), what=tag) as inst:
            drive(oracle, inst, [st], tag, seed + 31 * k)


# ---- the helper itself ------------------------------------------------------------------------------------------------------------

def test_a_byte_in_a_fence_is_noticed(guard):
    """the negative control: this test writes ONE byte into a fence, with torch, and the helper must raise -- at either end"""
    for where in (-1, 0):
        f = Fenced(guard.poison, 1000, skew=4)
        f.check("untouched")
        f.t[f.lo + where if where < 0 else f.lo + f.n] = guard.poison ^ 0x01
        with pytest.raises(AssertionError, match="front fence" if where < 0 else "back fence"):
            f.check("planted")
    f = Fenced(guard.poison, 1000)
    f.t[f.lo] = guard.poison ^ 0xFF                           # the region is the owner's to write
    f.t[f.lo + f.n - 1] = guard.poison ^ 0xFF
    f.check("inside")


def test_a_byte_in_a_band_is_noticed_on_the_device(guard, capfd):
    """the positive control of the mode itself, on the device: a buffer from the library's own allocator (sgmd_alloc, the one place
    every device buffer comes from) is poison from end to end; one byte written just behind it, then one just in front of it --
    inside the allocation the mode made, so nothing foreign is touched -- is counted and reported with its side and offset; a
    violated buffer that is freed leaves a count that the next check returns once"""
    import ctypes as C
    import soc_project_stereo_matching_amd as S
    L = S.load_library()
    L.sgmd_alloc.argtypes, L.sgmd_free.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_size_t], [C.c_int, C.c_void_p]
    L.sgmd_memset_async.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
    L.sgmd_d2h_async.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sgmd_stream_sync.argtypes = [C.c_int, C.c_void_p]
    n = 1001                                                  # no multiple of anything: the back band starts at an odd address
    p = C.c_void_p()
    assert L.sgmd_alloc(0, C.byref(p), n) == 0 and p.value and p.value % 4096 == 0

    def poke(offset, value):
        assert L.sgmd_memset_async(0, None, p.value + offset, value, 1) == 0 and L.sgmd_stream_sync(0, None) == 0

    try:
        host = np.zeros(n, np.uint8)
        assert L.sgmd_d2h_async(0, None, host.ctypes.data, p, n) == 0 and L.sgmd_stream_sync(0, None) == 0
        assert (host == guard.poison).all()                   # the payload is junk before its first use
        assert S.debug_guard_check() == (0, 1, n)
        capfd.readouterr()
        poke(n, guard.poison ^ 0x01)
        assert S.debug_guard_check() == (1, 1, n)
        assert f"payload of {n} bytes: back band written at +0 .. +0 " in capfd.readouterr().err
        poke(n, guard.poison)
        poke(n - 1, 0)                                        # the payload's last byte is the owner's
        assert S.debug_guard_check() == (0, 1, n)
        poke(n, guard.poison)                                 # THE blind spot: the poison itself (the other poison's run sees it)
        assert S.debug_guard_check() == (0, 1, n)
        poke(-1, guard.poison ^ 0x80)
        poke(-G, guard.poison ^ 0x80)
    finally:
        assert L.sgmd_free(0, p) == 0
    err = capfd.readouterr().err
    assert f"payload of {n} bytes: front band written at -{G} .. -1 " in err
    assert S.debug_guard_check() == (1, 0, 0)                 # found at the free, returned once
    assert S.debug_guard_check() == (0, 0, 0)


# ---- plain match --------------------------------------------------------------------------------------------------------------------

# (W, H, dmin, D): the tiny golden shapes; W < H; padded to 64; the census writes nothing; three widths round a wave; odd and
# wide; the padded ranges 192, 256, 512; one row; one column
PLAIN = [(24, 16, 0, 8), (20, 31, 0, 8), (40, 24, 3, 16), (64, 20, 0, 40), (5, 9, 0, 8), (9, 9, 0, 4), (63, 12, 0, 16), (64, 12, 0, 16),
         (65, 12, 0, 16), (257, 9, 2, 28), (200, 12, 0, 192), (200, 12, 0, 256), (70, 20, 0, 512), (64, 1, 0, 8), (1, 64, 0, 8)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("keep", [False, True], ids=["fast", "keep_stages"])
@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "separate_sum"])
def test_plain_match(guard, oracle, monkeypatch, fused, keep, batch):
    steps = [step(w, h, d, dmin=dmin, keep=keep, batch=batch) for (w, h, dmin, d) in PLAIN]
    drive_fresh(guard, oracle, monkeypatch, {"SGM_FUSED_WTA": fused}, steps, f"plain fused={fused}", 0x6A00 + batch)


# ---- large and out-of-range min_disparity: the longest look-behind into the census slack -----------------------------------------

@pytest.mark.parametrize("mode", ["default", "separate_sum", "batch3"])
@pytest.mark.parametrize("case", LM.DMIN_OUT + [LM.DMIN_IN_RANGE[0]], ids=LM.dmin_name)
def test_large_min_disparity(guard, oracle, monkeypatch, case, mode):
    from test_gpu_limits import check_all_stages, dmin_input, match_frames
    batch = 3 if mode == "batch3" else 1
    frames = [dmin_input(oracle, case, f) for f in range(batch)]
    env = {"SGM_FUSED_WTA": "0"} if mode == "separate_sum" else {}
    with guard.instances(fresh(monkeypatch, env, batch), what=LM.dmin_name(case)) as i:
        i.keep_stages(True)
        assert i.reset(case[0], case[1], LM.dmin_option(case))
        out = match_frames(i, [f[:2] for f in frames])
        assert out is not None
        for k, (_, _, want) in enumerate(frames):
            i.select_frame(k)
            check_all_stages(i, out[k], want, f"{LM.dmin_name(case)} {mode} frame {k}")


# ---- aggregation families and layouts -----------------------------------------------------------------------------------------------

AGG = {
    "plain_step": ({"SGM_AGG_FAST": "0"}, {}),
    "generic_negative_p1": ({}, dict(pen=(-5, 150))),
    "p_223_223": ({}, dict(pen=(223, 223))),
    "p_224_10": ({}, dict(pen=(224, 10))),
    "hl32": ({"SGM_HL": "32"}, {}),
    "hl64": ({"SGM_HL": "64"}, {}),
    "lanes8": ({"SGM_LANES_PER_PIXEL": "8"}, {}),
    "paths4": ({}, dict(paths4=True)),
}


@pytest.mark.parametrize("name", list(AGG))
def test_aggregation_families_and_layouts(guard, oracle, monkeypatch, name):
    env, kw = AGG[name]
    steps = [step(150, 25, 90, dmin=3, **kw), step(90, 33, 64, **kw), step(150, 25, 90, dmin=3, batch=3, **kw)]
    drive_fresh(guard, oracle, monkeypatch, env, steps, name, 0xA660)


@pytest.mark.parametrize("segments", [2, 3, 4])
def test_fused_sum_row_segments(guard, oracle, monkeypatch, segments):
    steps = [step(530, 20, 93, dmin=5), step(257, 9, 28, dmin=2)]
    drive_fresh(guard, oracle, monkeypatch, {"SGM_SUM_SEGMENTS": str(segments), "SGM_FUSED_WTA": "1"}, steps, f"segments={segments}", 0x5E60)


@pytest.mark.parametrize("rows", [3, 1])
def test_fused_last_sweep_on_a_fresh_instance(guard, oracle, monkeypatch, rows):
    """SGM_UPSUM=1: the scratch with the hand-over rows and the progress words is poison on first use -- a word the host did not
    initialise reads as "ahead" (0x5A...) or as -1, and a bounded poll that gives up refuses the match"""
    env = {"SGM_UPSUM": "1"}
    if rows != 3:
        env["SGM_UPSUM_ROWS"] = str(rows)

    def fused(i, k, tag):
        assert i.fused_sweep_rows() == rows, tag

    for st in (step(161, 20, 128, dmin=3, batch=2), step(130, 16, 128)):
        tag = f"fused sweep rows={rows} {st['w']}x{st['h']} b{st['batch']}"
        with guard.instances(new_instance(monkeypatch, env), what=tag) as inst:
            drive(oracle, inst, [st], tag, 0x0F5E + rows, after=fused)


@pytest.mark.parametrize("name,kw", [("centre9x7_u64", dict(window=(9, 7))), ("symmetric7x7", dict(kind=SYMMETRIC, window=(7, 7)))])
def test_census_variants(guard, oracle, monkeypatch, name, kw):
    steps = [step(130, 47, 48, dmin=2, **kw), step(130, 47, 48, dmin=2, keep=True, **kw), step(130, 47, 48, dmin=2, batch=3, **kw)]
    drive_fresh(guard, oracle, monkeypatch, {}, steps, name, 0xCE50)


# ---- views and extras ---------------------------------------------------------------------------------------------------------------

EXTRAS = {
    "right_view": dict(view=True),
    "match_both": dict(entry="both"),
    "match_both_keep": dict(entry="both", keep=True),
    "confidence": dict(entry="confidence"),
    "fill": dict(fill=True),
    "fill_right_view": dict(fill=True, view=True),
    "refine": dict(refine=True),
    "confidence_batch3": dict(entry="confidence", batch=3),
    "both_batch3": dict(entry="both", batch=3),
}


@pytest.mark.parametrize("name", list(EXTRAS))
def test_views_and_extras(guard, oracle, monkeypatch, name):
    steps = [step(70, 33, 16, **EXTRAS[name]), step(96, 64, 64, **EXTRAS[name])]
    drive_fresh(guard, oracle, monkeypatch, {}, steps, name, 0xE7A0)


@pytest.mark.parametrize("how", ["overlap_post", "stage_cus"])
def test_post_pass_on_a_stream_of_its_own(guard, oracle, monkeypatch, how):
    for st in (step(70, 33, 16, batch=2), step(96, 64, 64, fill=True)):
        inst = new_instance(monkeypatch, {})
        with guard.instances(inst, what=how):
            if how == "overlap_post":
                assert inst.set_overlap_post(True)
            else:
                assert inst.set_cu_split("post=0:4,main=4:28")
            drive(oracle, inst, [st], how, 0x0B50)


# ---- rectification ------------------------------------------------------------------------------------------------------------------

def shifted_maps(w, h, dx, dy):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x + dx, y + dy, x - dx, y - dy                     # taps outside the source on every side, left and right differently


@pytest.mark.parametrize("batch", [1, 3])
def test_rectification_with_taps_outside_the_source(guard, oracle, monkeypatch, batch):
    steps = [step(70, 33, 16, rect=shifted_maps(70, 33, 3, -3), batch=batch), step(96, 64, 64, rect=shifted_maps(96, 64, -3, 3), batch=batch),
             step(65, 17, 16, rect=RR.model_maps(RR.SMALL, 65, 17) + RR.model_maps(RR.SMALL, 65, 17, sign=-1.0), batch=batch)]
    drive_fresh(guard, oracle, monkeypatch, {}, steps, "rectify 8 bit", 0x4EC0)


def test_rectification_of_12_bit_images(guard, oracle, monkeypatch):
    """u16 = u8 << 4 under whole-pixel shifts: the remap copies samples or writes 0, so every stage is the oracle's on the 8-bit
    remap (the shift identity of tests/test_gpu_pixels16.py), and stages 19 / 20 are pixels16_ref's remap of the u16 images"""
    w, h, d = 70, 33, 16
    maps = shifted_maps(w, h, 3, -3)
    l8, r8 = oracle.synth_pair(w, h, d, 0x4EC12)
    opt = default_option(d, min_speckle_area=10)
    want = oracle.run(RR.remap(l8, *maps[:2]), RR.remap(r8, *maps[2:]), opt)
    l16, r16 = P.widen(l8, 12), P.widen(r8, 12)
    with guard.instances(fresh(monkeypatch), what="rectify 12 bit") as i:
        i.keep_stages(True)
        assert i.set_pixel_bits(12) and i.set_rectify(*maps) and i.reset(w, h, opt)
        out = i.match(l16, r16)
        assert out is not None
        got = i.read_stages()
        for n, v in want.items():
            assert_same(got[n], v, f"12 bit rectified: {n}")
        assert_same(out, want["final"], "12 bit rectified: result")
        got_l, got_r = i.read_rectified()
        assert_same(got_l, P.remap(l16, *maps[:2]), "stage 19")
        assert_same(got_r, P.remap(r16, *maps[2:]), "stage 20")


def test_match_planes_with_an_odd_pitch(guard, oracle, monkeypatch):
    """322 x 97: W * H % 4 == 2, so the frames of a batch of 3 start on no dword boundary in the grey and rectified images"""
    from oracle.platform_oracle import board_gray, disparity_to_depth
    from test_gpu_parity import _colour_planes
    from test_gpu_rectify import Rig
    w, h, d = 322, 97, 32
    fx, baseline, doffs = 1733.74, 536.62, 0.0
    rng = np.random.default_rng(322)
    planes = np.stack([_colour_planes(oracle, w, h, d, 0x4EF0 + k, rng) for k in range(3)])
    rig = Rig(w, h)
    with guard.instances(fresh(monkeypatch, batch=3), what="match_planes") as i:
        assert rig.on(i) and i.reset(w, h, default_option(d))
        depth = np.empty((3, h, w), np.float32)
        assert i.match_planes(np.ascontiguousarray(planes), fx, baseline, doffs, depth)
        for k in range(3):
            grey = board_gray(*planes[k, :3]), board_gray(*planes[k, 3:])
            disp = oracle.run(*rig.rectified(*grey), default_option(d))["final"]
            i.select_frame(k)
            assert_same(i.read_stage("final"), disp, f"frame {k}: disparity behind the depth map")
            want = disparity_to_depth(disp, fx, baseline, doffs)
            assert np.array_equal(np.isnan(depth[k]), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(depth[k][ok].view(np.uint32), want[ok].view(np.uint32)), f"frame {k}: depth"


# ---- 12- and 16-bit images --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [12, 16])
def test_pixels16(guard, oracle, monkeypatch, pairs8, bits):  # noqa: F811
    """the shift identity of tests/test_gpu_pixels16.py at two of its shapes: 70x33, and 131x21 as a batch of three (W * H odd)"""
    import test_gpu_pixels16 as T
    for shape in (T.SHAPES[0], T.SHAPES[3]):
        w, h, _, _, B = shape
        l8, r8 = pairs8[shape]
        opt = T.options(shape)
        with guard.instances(fresh(monkeypatch, batch=B), what=f"{bits} bit {shape}") as i:
            i.keep_stages(True)
            assert i.set_pixel_bits(bits) and i.reset(w, h, opt)
            out = i.match(T.squeeze(P.widen(l8, bits), B), T.squeeze(P.widen(r8, bits), B))
            assert out is not None
            T.check_frames(i, out, lambda k: oracle.run(l8[k], r8[k], opt), B, f"shift {shape} {bits} bits")
            for k in range(B):
                i.select_frame(k)
                gl, gr = i.read_narrowed()
                assert_same(gl, l8[k], "g8 left")
                assert_same(gr, r8[k], "g8 right")


# ---- growth and shrink under poison -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["default", "batch3", "keep_stages", "both", "q14"])
def test_shape_ladder(guard, oracle, monkeypatch, mode):
    """the ladder of tests/test_gpu_instance_reuse.py on ONE instance: every buffer that grows is junk before its first use, and the
    buffer it replaces is verified as it is freed"""
    kw = {"default": {}, "batch3": dict(batch=3), "keep_stages": dict(keep=True), "both": dict(entry="both"), "q14": dict(q14=True)}[mode]
    assert len(LADDER) == 6
    with guard.instances(new_instance(monkeypatch, {}), what=f"ladder {mode}") as inst:
        drive(oracle, inst, ladder(kw), f"ladder {mode}", 0x1AD0 + len(mode))


# ---- row tiles ----------------------------------------------------------------------------------------------------------------------

def test_row_tiles_of_one_frame_on_one_instance(guard, oracle, monkeypatch):
    """the top / bottom sequence of tests/test_gpu_instance_reuse.py: in row-tile mode the plane pointer lies IN FRONT of its
    allocation (the rows above the tile do not exist); the hand-over buffers are the caller's, exactly tile_boundary_bytes() long"""
    import torch
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")
    with guard.instances(new_instance(monkeypatch, {}), what="row tiles") as inst:
        for (w, h, d) in ((130, 48, 64), (77, 48, 64)):
            opt = default_option(d, min_speckle_area=10)
            left, right = oracle.synth_pair(w, h, d, 0x7113 + w)
            want = oracle.run(left, right, opt)
            f_l, f_r = guard.buf(left), guard.buf(right)
            f_disp, f_disp_b = guard.buf(4 * w * h), guard.buf(4 * w * h)
            top, bottom = (0, h // 2), (h // 2, h)
            assert inst.set_rows(*top) and inst.reset(w, h, opt)
            f_fwd, f_bwd = guard.buf(inst.tile_boundary_bytes()), guard.buf(inst.tile_boundary_bytes())

            class Ptr:                                        # what _tile asks of a tensor
                def __init__(self, f):
                    self.f = f

                def data_ptr(self):
                    return self.f.ptr

            dl, dr, disp, disp_b, fwd, bwd = (Ptr(f) for f in (f_l, f_r, f_disp, f_disp_b, f_fwd, f_bwd))
            assert not _tile(inst, top, w, h, opt, dl, dr, disp, {}, {True: fwd})
            assert inst.synchronize()
            assert _tile(inst, bottom, w, h, opt, dl, dr, disp_b, {True: fwd}, {False: bwd})
            assert_same(inst.read_stage("aggr")[h // 2:], want["aggr"][h // 2:], f"{w}x{h}: S of the bottom tile")
            assert _tile(inst, top, w, h, opt, dl, dr, disp, {False: bwd}, {})
            assert_same(inst.read_stage("aggr")[:h // 2], want["aggr"][:h // 2], f"{w}x{h}: S of the top tile")
            whole = f_disp.get(np.float32, (h, w))
            whole[h // 2:] = f_disp_b.get(np.float32, (h, w))[h // 2:]
            f_all = guard.buf(whole)
            torch.cuda.synchronize()
            assert inst.tile_post(f_all.ptr) and inst.synchronize()
            assert_same(f_all.get(np.float32, (h, w)), want["final"], f"{w}x{h}: the gathered map")
            assert_same(f_l.get(np.uint8, (h, w)), left, "the left image is only read")
            guard.check_fences(f"row tiles {w}x{h}")
            assert inst.set_rows(0, 0) and inst.reset(w, h, opt)
            assert_same(inst.match(left, right), want["final"], f"{w}x{h}: a plain match after the tiles")


def test_three_row_tiles_in_one_process(guard, oracle, monkeypatch):
    import torch
    from soc_project_stereo_matching_amd.tiling import match_tiled_in_process
    from test_gpu_limits import tile_engines
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")
    w, h, d = 130, 50, 64
    opt = default_option(d, min_speckle_area=10)
    left, right = oracle.synth_pair(w, h, d, 0x7133)
    want = oracle.run(left, right, opt)
    engines = tile_engines(w, h, opt, 3)
    with guard.instances(*[e.inst for e in engines], what="three tiles"):
        got = match_tiled_in_process(engines, torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda())
        assert_same(got.cpu().numpy(), want["final"], "three row tiles")
        for e in engines:
            r0, r1 = e.rows
            assert_same(e.inst.read_stage("aggr")[r0:r1], want["aggr"][r0:r1], f"S rows {r0}:{r1}")


# ---- the post pass on crafted maps ---------------------------------------------------------------------------------------------------

def post_through_fences(guard, inst, oracle, w, h, maps, area, what, median_only=False):
    import soc_project_stereo_matching_amd as S
    assert inst.reset(w, h, S.default_option(16, min_speckle_area=area, is_remove_speckles=not median_only))
    for name, m in maps.items():
        want = oracle.median(m.copy() if median_only else oracle.remove_speckles(m.copy(), area))
        for rep in range(2):
            f = guard.buf(m)
            assert inst.tile_post(f.ptr) and inst.synchronize()
            assert_same(f.get(np.float32, (h, w)), want, f"{what} {name} {w}x{h} min_area={area} visit {rep}")
    guard.check_fences(what)


@pytest.mark.parametrize("tile_rows", [16, 64])
@pytest.mark.parametrize("shape", [(65, 33), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_speckle_and_median_on_crafted_maps(guard, oracle, monkeypatch, shape, tile_rows):
    from test_gpu_parity import _speckle_maps
    w, h = shape
    maps = _speckle_maps(np.random.default_rng(w * 1000 + h), h, w)
    with guard.instances(fresh(monkeypatch, {"SGM_SPECKLE_TILE_ROWS": tile_rows}), what=f"post {w}x{h}") as i:
        for area in (1, 50, 65535):
            post_through_fences(guard, i, oracle, w, h, maps, area, f"tile rows {tile_rows}")


def _median_chain_child(chain, poison):
    """SGM_MEDIAN_CHAIN is read once per process, at the first median launch: the tall maps in a process of their own"""
    from test_gpu_parity import _speckle_maps
    assert os.environ["SGM_MEDIAN_CHAIN"] == chain and os.environ["SGM_DEBUG_GUARD"] == str(G)
    import soc_project_stereo_matching_amd as S
    guard, oracle = Guard(poison), Oracle()
    with guard.instances(S.SGMInstance(0), what=f"chain={chain}") as i:
        for (w, h) in ((40, 1100), (24, 515), (40, 1100)):    # 5 bands, 3 bands, 5 again: the granule rows move within the scratch
            maps = _speckle_maps(np.random.default_rng(w + h), h, w)
            post_through_fences(guard, i, oracle, w, h, {n: maps[n] for n in ("ramp", "noise_thr", "holes")}, 0, f"chain={chain}",
                                median_only=True)
    print("median chain child ok")


@pytest.mark.parametrize("chain", ["1", "0"])
def test_chained_median_of_tall_maps(guard, chain):
    env = dict(os.environ, SGM_MEDIAN_CHAIN=chain,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "median_chain", chain, str(guard.poison)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "median chain child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- caller-owned device memory: the _device entry points ---------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["match", "confidence", "both"])
def test_device_entry_points(guard, oracle, monkeypatch, entry):
    """images one byte off an aligned base, maps one float off; inputs fenced too: a result that depends on bytes beyond an image
    differs between the two poisons"""
    for (w, h, d, batch) in ((70, 33, 16, 1), (65, 17, 16, 3)):
        st = step(w, h, d, batch=batch, entry=entry)
        opt = option_of(st)
        pairs, L, R = frames_of(oracle, st, 0xDE70 + w)
        n = batch * w * h
        with guard.instances(fresh(monkeypatch, batch=batch), what=f"{entry}_device {w}x{h}") as i:
            assert i.reset(w, h, opt)
            f_l, f_r = guard.buf(L, skew=1), guard.buf(R, skew=1)
            outs = [guard.buf(4 * n, skew=4)]
            if entry == "confidence":
                outs.append(guard.buf(2 * n, skew=2))
                assert i.match_confidence_device(f_l.ptr, f_r.ptr, outs[0].ptr, outs[1].ptr)
            elif entry == "both":
                outs.append(guard.buf(4 * n, skew=4))
                assert i.match_both_device(f_l.ptr, f_r.ptr, outs[0].ptr, outs[1].ptr)
            else:
                assert i.match_device(f_l.ptr, f_r.ptr, outs[0].ptr)
            assert i.synchronize()
            for j, (l, r) in enumerate(pairs):
                want = expected(oracle, st, opt, l, r)
                assert_same(outs[0].get(np.float32, (batch, h, w))[j], want["final"], f"{entry} frame {j}: map")
                if entry == "confidence":
                    assert_same(outs[1].get(np.uint16, (batch, h, w))[j], want["conf"], f"frame {j}: confidence")
                if entry == "both":
                    assert_same(outs[1].get(np.float32, (batch, h, w))[j], want["final_r"], f"frame {j}: right map")
            assert_same(f_l.get(np.uint8, L.shape), L, "the left images are only read")
            assert_same(f_r.get(np.uint8, R.shape), R, "the right images are only read")


# ---- scaled match -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,f", [(67, 19, 2), (70, 23, 4)])
def test_downscale_and_upscale_alone(guard, monkeypatch, W, H, f):
    import soc_project_stereo_matching_amd as S
    from test_gpu_scaled import planted, same, spec_of
    rng = np.random.default_rng(W * 1000 + H)
    with guard.instances(fresh(monkeypatch), what=f"scale {W}x{H} f={f}") as i:
        assert i.reset(24, 16, default_option(8))             # (neither kernel needs it: the library's own buffers are live beside them)
        for bits in (8, 12):
            dt = np.uint16 if bits > 8 else np.uint8
            sp = spec_of(W, H, f, frames=3, bits=bits)
            img = rng.integers(0, 1 << bits, (3, H, W)).astype(dt)
            want = SR.downscale(img, f)
            for off in (0, 1):
                src, out = guard.buf(img, skew=off * dt().itemsize), guard.buf(want.nbytes)
                assert i.downscale(sp, src.ptr, out.ptr) and i.synchronize()
                same(out.get(dt, want.shape), want, f"downscale {bits} bits offset {off}")
                same(src.get(dt, img.shape), img, "the source is only read")
        d_lo, d_hi = 3, 3 + (W * 2) // 3
        for radius, right, inf_share in ((3, False, 0.3), (4, True, 0), (-1, False, 0.3), (0, True, 1)):
            arrays = planted(rng, W, H, f, 2, 8, inf_share, d_hi + 2 * f)
            sp = spec_of(W, H, f, frames=2, bits=8, radius=radius, penalty=1, d_lo=d_lo, d_hi=d_hi)
            dev = [guard.buf(a) for a in arrays]
            out = guard.buf(4 * arrays[2].size)
            planes = (dev[3].ptr, dev[4].ptr) if radius >= 0 else (None, None)
            assert i.upscale_disparity(sp, dev[0].ptr, dev[1].ptr, dev[2].ptr, planes[0], planes[1], right, out.ptr) and i.synchronize()
            want = SR.upscale_batch(*arrays, sp.factor, sp.radius, sp.penalty, sp.d_lo, sp.d_hi, right)
            same(out.get(np.float32, want.shape), want, f"upscale r={radius} right={right} inf={inf_share}")
        assert S.scaled_shape(sp) == (W // f, H // f)


@pytest.mark.parametrize("W,H,f", [(67, 19, 2), (70, 23, 4)])
def test_match_scaled(guard, oracle, monkeypatch, W, H, f):
    """host form and device form (fenced images and map) against scaled_ref on the oracle's small map"""
    import soc_project_stereo_matching_amd as S
    from test_gpu_scaled import full_words, same, scene, small_finals, spec_of
    w, h, D, B = W // f, H // f, 8, 2
    opt = default_option(D, 0, min_speckle_area=9)
    left, right = scene(W, H, f * 6, B, 8, 4242 + W)
    ls, rs = SR.downscale(left, f), SR.downscale(right, f)
    small = np.stack([small_finals(oracle, ls[k], rs[k], opt, 8, False, False) for k in range(B)])
    words_l = np.stack([full_words(oracle, left[k], 8, False) for k in range(B)])
    words_r = np.stack([full_words(oracle, right[k], 8, False) for k in range(B)])
    want = SR.upscale_batch(small, ls, left, words_l, words_r, f, S.sgm.SCALE_DEFAULT_RADIUS, S.sgm.SCALE_DEFAULT_PENALTY, 0, f * D - 1, False)
    sp = spec_of(W, H, f, frames=B, bits=8)
    with guard.instances(fresh(monkeypatch, batch=B), what=f"match_scaled {W}x{H} f={f}") as i:
        assert i.initialize(w, h, opt)
        got = i.match_scaled(sp, left, right)
        assert got is not None
        same(got.reshape(want.shape), want, "host form")
        for k in range(B):
            i.select_frame(k)
            same(i.read_stage(8), small[k], f"stage 8 of frame {k}")
        assert i.reset(w, h, opt)
        f_l, f_r, out = guard.buf(left, skew=1), guard.buf(right, skew=1), guard.buf(want.nbytes, skew=4)
        assert i.match_scaled_device(sp, f_l.ptr, f_r.ptr, out.ptr) and i.synchronize()
        same(out.get(np.float32, want.shape), want, "device form")
        same(f_l.get(np.uint8, left.shape), left, "the left images are only read")


# ---- temporal filter ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pixels", [1, 3, 143, 4096])
def test_temporal_kernel_alone(guard, monkeypatch, pixels):
    from test_gpu_temporal import c_spec
    with guard.instances(fresh(monkeypatch), what=f"temporal {pixels} pixels") as i:
        for k, spec in enumerate(TC.PARAMS[:2]):
            for (streams, steps, skew) in ((1, 1, 0), (2, 3, 1)):
                shape = (pixels, streams, steps, bool(skew))
                maps, conf, hv, hb = TC.inputs(shape, spec)
                for with_conf in (True, False):
                    want = TR.run(spec, maps, conf if with_conf else None, hv, hb)
                    what = f"{TC.shape_id(shape)} {spec} conf={with_conf}"
                    f_maps, f_conf = guard.buf(maps, skew=4 * skew), guard.buf(conf, skew=2 * skew)
                    f_hv, f_hb, f_st = guard.buf(hv), guard.buf(hb), guard.buf(streams * steps * 5 * 4)
                    assert i.temporal_filter(c_spec(spec), streams, steps, pixels, f_maps.ptr, f_conf.ptr if with_conf else None,
                                             f_hv.ptr, f_hb.ptr, f_st.ptr), what
                    assert i.synchronize()
                    assert_same(f_maps.get(np.float32, maps.shape), want[0], what + ": maps")
                    assert_same(f_hv.get(np.float32, hv.shape), want[1], what + ": hv")
                    assert_same(f_hb.get(np.uint8, hb.shape), want[2], what + ": hb")
                    assert_same(f_st.get(np.uint32, want[3].shape), want[3], what + ": counters")
                    assert_same(f_conf.get(np.uint16, conf.shape), conf, what + ": the confidence is only read")
                    guard.check_fences(what)


@pytest.mark.parametrize("how", ["three_calls", "sequence_batch", "three_streams"])
def test_temporal_through_the_match(guard, oracle, golden_cases, how):
    """70 x 33: three single-frame calls, one sequence batch of three, one batch of three streams (tests/test_gpu_temporal.py)"""
    import test_gpu_temporal as T
    from conftest import case_inputs, option_from_dict
    name = "t70x33_d16"
    opt, frames, finals, rows = T.sequence(oracle, golden_cases, name)
    h, w = finals[0].shape
    if how == "three_calls":
        with guard.instances(T.make(), what=how) as i:
            for k, (l, r) in enumerate(frames[:3]):
                assert i.reset(w, h, opt)
                got = i.match(l, r)
                assert got is not None
                assert_same(i.read_stage(29), finals[k], f"frame {k}: stage 29")
                assert_same(got, rows[k][0], f"frame {k}: the returned map")
                T.check_state(i, rows[k], f"frame {k}")
                assert_same(i.temporal_stats(), rows[k][3].reshape(1, 5), f"frame {k}: counters")
    elif how == "sequence_batch":
        with guard.instances(T.make(batch=3, sequence_mode=1), what=how) as i:
            assert i.reset(w, h, opt)
            got = i.match(np.stack([p[0] for p in frames[:3]]), np.stack([p[1] for p in frames[:3]]))
            assert got is not None
            for f in range(3):
                i.select_frame(f)
                assert_same(i.read_stage(29), finals[f], f"frame {f}: stage 29")
                assert_same(got[f], rows[f][0], f"frame {f}: the returned map")
                T.check_state(i, rows[2], f"read through frame {f}")
            assert_same(i.temporal_stats(), np.stack([rows[f][3] for f in range(3)]), "counters")
    else:
        case = golden_cases[name]
        left, right = case_inputs(case, oracle)
        streams = [TC.frames_of(left, right, first=10 * s, count=2, blank=10 * s + 1 if s == 1 else -1) for s in range(3)]
        srows = [TC.filtered(T.SPEC, [oracle.run(l, r, opt)["final"] for l, r in fr]) for fr in streams]
        with guard.instances(T.make(batch=3), what=how) as i:
            for call in range(2):
                assert i.reset(w, h, opt)
                got = i.match(np.stack([streams[s][call][0] for s in range(3)]), np.stack([streams[s][call][1] for s in range(3)]))
                for s in range(3):
                    i.select_frame(s)
                    assert_same(got[s], srows[s][call][0], f"stream {s} call {call}")
                    T.check_state(i, srows[s][call], f"stream {s} call {call}")
                assert_same(i.temporal_stats(), np.stack([srows[s][call][3] for s in range(3)]), f"call {call}: counters")


# ---- clouds, depth, grey --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 3])
def test_clouds(guard, monkeypatch, frames):
    """organised and compacted clouds at 70 x 33: all-invalid, mixed and all-valid frames; the point list holds exactly total
    records -- those past the total stay poison, as include/sgm_mi355x.h promises"""
    from test_gpu_cloud import c_spec, make_spec, maps_for
    w, h = 70, 33
    n = frames * w * h
    rng = np.random.default_rng(70 + frames)
    s = make_spec(w, h, frames=frames)
    kinds = {"all invalid": np.zeros(n, bool), "mixed": rng.random(n) < 0.5, "all valid": np.ones(n, bool)}
    if frames == 3:
        kinds["invalid / mixed / valid"] = np.concatenate([np.zeros(w * h, bool), rng.random(w * h) < 0.5, np.ones(w * h, bool)])
    with guard.instances(fresh(monkeypatch), what=f"clouds {frames} frames") as i:
        for label, keep in kinds.items():
            for side_maps in (True, False):
                disp, mask, conf = maps_for(keep, (frames, h, w), rng, non_finite=label == "mixed")
                if not side_maps:
                    mask = conf = None
                f_disp = guard.buf(disp, skew=4)
                f_mask = guard.buf(mask, skew=1) if side_maps else None
                f_conf = guard.buf(conf, skew=2) if side_maps else None
                f_xyz, f_pts, f_off, f_depth = guard.buf(12 * n), guard.buf(16 * n), guard.buf(4 * (frames + 1)), guard.buf(4 * n, skew=4)
                p_mask, p_conf = (f_mask.ptr, f_conf.ptr) if side_maps else (None, None)
                cs = c_spec(s)
                assert i.cloud_organized(cs, f_disp.ptr, p_mask, p_conf, f_xyz.ptr), label
                assert i.cloud_points(cs, f_disp.ptr, p_mask, p_conf, f_pts.ptr, f_off.ptr), label
                assert i.disparity_to_depth(f_disp.ptr, n, s.fx, s.baseline, s.doffs, f_depth.ptr) and i.synchronize(), label
                want_pts, want_off = CLR.points(disp, s, mask, conf)
                want_org = CLR.organized(disp, s, mask, conf)
                kept, _ = CLR.kept(disp, s, mask, conf)
                total = int(want_off[-1])
                assert total == kept.sum() and (not side_maps or np.array_equal(kept.reshape(-1), keep))
                assert_same(f_off.get(np.uint32), want_off, f"{label}: offsets")
                raw = f_pts.get(np.uint8)
                assert raw[:16 * total].tobytes() == want_pts.tobytes(), f"{label}: the point list"
                assert np.all(raw[16 * total:] == guard.poison), f"{label}: a record at index total or beyond was written"
                got_org = f_xyz.get(np.uint32, want_org.shape)
                assert np.array_equal(got_org, want_org.view(np.uint32)), f"{label}: organised cloud"
                depth = f_depth.get(np.uint32).reshape(kept.shape)
                assert np.array_equal(got_org[..., 2][kept], depth[kept]), f"{label}: Z is not sgm_disparity_to_depth's"
                assert f_disp.get(np.float32, disp.shape).tobytes() == disp.tobytes(), "the map is only read"
                guard.check_fences(label)


@pytest.mark.parametrize("n", [3, 1001])
def test_depth_and_grey(guard, monkeypatch, n):
    from oracle.platform_oracle import board_gray, compare_depth, disparity_to_depth
    rng = np.random.default_rng(n)
    fx, baseline, doffs = 3979.911, 193.001, 124.343
    disp = rng.uniform(0, 64, n).astype(np.float32)
    disp[rng.random(n) < 0.2] = np.inf
    disp[0] = np.float32(-doffs)
    with guard.instances(fresh(monkeypatch), what=f"depth and grey n={n}") as i:
        assert i.reset(24, 16, default_option(8))             # (none of the three needs it: the library's own buffers are live beside them)
        f_disp, f_depth = guard.buf(disp, skew=4), guard.buf(4 * n, skew=4)
        assert i.disparity_to_depth(f_disp.ptr, n, fx, baseline, doffs, f_depth.ptr) and i.synchronize()
        got, want = f_depth.get(np.float32), disparity_to_depth(disp, fx, baseline, doffs)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
        # scoring: the per-block partials are a device buffer of the library's own (allocated and freed inside the call)
        gt = (want + rng.normal(0, 8, n).astype(np.float32)).astype(np.float32)
        gt[rng.random(n) < 0.1] = np.nan
        f_gt, f_test = guard.buf(gt, skew=4), guard.buf(want, skew=4)
        rmse, bpr, valid = i.compare_depth(f_gt.ptr, f_test.ptr, n, 10.0)
        w_rmse, w_bpr, w_n = compare_depth(gt, want, 10.0)
        assert valid == w_n
        if w_n:
            assert abs(bpr - w_bpr) < 1e-12 and abs(rmse - w_rmse) <= 1e-6 * w_rmse
        for weight_r in (76, 77):
            bgr = rng.integers(0, 256, (3, n), dtype=np.uint8)
            bgr[:, :3] = [[255, 0, 255], [255, 0, 0], [255, 255, 0]]
            f_bgr, f_grey = guard.buf(bgr), guard.buf(n)
            assert i.gray_from_planes(f_bgr.ptr, n, f_grey.ptr, weight_r) and i.synchronize()
            assert_same(f_grey.get(np.uint8), board_gray(bgr[0], bgr[1], bgr[2], weight_r), f"grey, weight {weight_r}")
            assert_same(f_bgr.get(np.uint8, bgr.shape), bgr, "the planes are only read")


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "median_chain":
    _median_chain_child(sys.argv[2], int(sys.argv[3]))
