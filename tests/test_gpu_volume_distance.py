"""The distance field of the TSDF volume on the device (extension; include/sgm_mi355x.h, the distance section) against the numpy
restatement tests/distance_ref.py -- needs an MI355X.  Tolerance 0 everywhere: words and bytes are compared.  Every array a call may
write sits between margins of 0xA5 and is pre-filled with it (or, where the test says so, with 0x00), the margins are checked
afterwards and the inputs compared unchanged.  The cases are those of tests/test_distance_cpu.py, which holds them against brute
force on the restatement alone."""
import itertools

import numpy as np
import pytest

import distance_ref as DR
import volume_ref as VR
import window_ref as WR
from geometry_large import constant
from test_distance_cpu import (DENSITIES, SMALL_DIMS, ball_scene, check_ball, check_rim, fused_reference, fused_scene, one_site, planted_words,
                               rim_cases, small_cases)
from test_gpu_raycast import MARGIN, Between
from test_gpu_volume import c_source, c_volume, upload

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

FAR = DR.FAR
ROW_WAVE = constant("sgm_distance.hip", "DIST_ROW_WAVE")
LINE_TIERS = [constant("sgm_distance.hip", "DIST_LINE_" + t) for t in "ABCD"]


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: the distance field needs no shape
    yield i
    i.close()


def spec_of(dims, voxel=0.0625):
    return VR.spec(*dims, voxel, (-1.125, -1.0, 0.5), 0.25)


class Off(Between):
    """Between, `off` bytes further on: a 16-bit array 2 bytes off a 16-byte boundary; fill: what an output holds beforehand"""
    def __init__(self, nbytes, data=None, off=0, fill=0xA5):
        super().__init__(nbytes, data)
        self.off = MARGIN + off
        if off or fill != 0xA5 or data is not None:
            self.hold[:] = 0xA5
            if data is not None:
                self.hold[self.off:self.off + nbytes].copy_(self.torch.from_numpy(np.array(data).reshape(-1).view(np.uint8)))
            elif fill != 0xA5:
                self.hold[self.off:self.off + nbytes] = fill


def device_distance(inst, v, words, min_weight, r, side, unknown, label, d_vox=None, out=None, skew=(0, 0), fill=0xA5):
    """one call: the words written, uint16 [nz][ny][nx]; d_vox: the volume on the device, made here (and checked as only read)
    unless given; out: the output array, made here unless given"""
    import torch
    import soc_project_stereo_matching_amd as S
    own = d_vox is None
    if own:
        d_vox = Off(words.nbytes, words, off=skew[0])
    if out is None:
        out = Off(2 * words.size, off=skew[1], fill=fill)
    torch.cuda.synchronize()
    assert inst.volume_distance(c_volume(v), S.distance_spec(min_weight, r, side, unknown), d_vox.ptr, out.ptr) and inst.synchronize(), label
    got = out.read(label, np.uint16).reshape(words.shape).copy()
    if own:
        assert d_vox.read(label + " volume").tobytes() == np.ascontiguousarray(words).tobytes(), f"{label}: the volume is only read"
    return got


def same_words(label, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k, j, i = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {got.size} words differ, first at (i, j, k) = ({i}, {j}, {k}): {int(got[k, j, i])} for {int(want[k, j, i])}")


def check(inst, dims, words, min_weight, r, side, unknown, label, **kw):
    got = device_distance(inst, spec_of(dims), words, min_weight, r, side, unknown, label, **kw)
    same_words(label, got, DR.distance(words, min_weight, r, side, unknown))
    return got


# ---- 1. every edge -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SMALL_DIMS)
def test_every_edge_of_the_small_volumes(inst, dims):
    calls = 0
    for d, density, min_weight, words in small_cases():
        if d != dims:
            continue
        d_vox = Off(words.nbytes, words)
        for r, side, unknown in itertools.product((1, 2, 3, 255), (0, 1), (0, 1)):
            check(inst, dims, words, min_weight, r, side, unknown, f"{dims} density {density} min_weight {min_weight} r={r} side={side} unknown={unknown}",
                  d_vox=d_vox)
            calls += 1
        assert d_vox.read("volume").tobytes() == words.tobytes()
    assert calls == len(DENSITIES) * 16


def test_the_rim_of_the_radius_in_the_middle_and_in_every_corner(inst):
    for words, site, checks in rim_cases():
        got = check(inst, (13, 13, 13), words, 1, 5, 0, 0, f"site {site}")
        check_rim(got, site, checks)


# ---- 2. the tiers of the launcher ----------------------------------------------------------------------------------------------

def tier_words(dims, seed, density=0.003):
    return planted_words(np.random.default_rng(seed), dims, density, 1)


@pytest.mark.parametrize("nx", [ROW_WAVE - 1, ROW_WAVE, ROW_WAVE + 1, 2 * ROW_WAVE + 1, 132, 1024])
def test_row_lengths_around_every_tier_of_the_x_pass(inst, nx):
    """rows that share a wave, one that fills it, rows of a wave's own by element and four voxels per lane, the longest"""
    dims = (nx, 3, 5)
    words = tier_words(dims, nx, 0.02)
    for r, side, unknown in ((1, 0, 0), (40, 0, 0), (255, 0, 0), (255, 1, 1), (33, 1, 0)):
        check(inst, dims, words, 1, r, side, unknown, f"{dims} r={r} side={side} unknown={unknown}")
    # a row with one site at either end, a row without one, a row that is all sites
    words = np.full((5, 3, nx), 0x00010005, np.uint32)
    words[0, 0, 0] = words[1, 1, nx - 1] = words[2, 2, nx // 2] = 0x00018000
    words[4, 1, :] = 0x00018000
    for r in (1, 31, 32, 64, 255):
        check(inst, dims, words, 1, r, 0, 0, f"{dims} planted rows r={r}")


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("length", sorted({t + o for t in LINE_TIERS for o in (-1, 0, 1)}))
def test_line_lengths_around_every_strip_width(inst, axis, length):
    """ny (the y pass) and nz (the z pass) just below, at and above every threshold of the strip width, with rows that take the
    16-byte loads of the strip (nx = 24) and rows that do not (nx = 9)"""
    for nx in (24, 9):
        dims = (nx, length, 2) if axis == 1 else (nx, 2, length)
        words = tier_words(dims, 7 * length + nx)
        for r, side in ((7, 0), (255, 0), (3, 1)):
            check(inst, dims, words, 1, r, side, 0, f"{dims} r={r} side={side}")


@pytest.mark.parametrize("dims", [(64, 1024, 2), (64, 2, 1024), (1024, 2, 2), (300, 70, 3)])
def test_the_longest_lines_at_the_largest_radius(inst, dims):
    words = tier_words(dims, sum(dims), 0.0005)
    check(inst, dims, words, 1, 255, 0, 0, f"{dims} r=255")
    check(inst, dims, words, 1, 255, 1, 1, f"{dims} r=255, the complement with unknown space")


def test_lines_shorter_than_the_radius(inst):
    for dims in ((5, 4, 3), (70, 6, 2), (8, 2, 9), (2, 2, 2)):
        words = tier_words(dims, 5 + sum(dims), 0.05)
        for r in (10, 100, 255):
            check(inst, dims, words, 1, r, 0, 0, f"{dims} r={r}")


# ---- 3. alignment and independence ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(136, 9, 5), (48, 9, 5), (137, 3, 3)])
def test_arrays_off_their_16_byte_boundaries_give_the_same_bytes(inst, dims):
    words = tier_words(dims, 11 + dims[0], 0.01)
    want = DR.distance(words, 1, 9, 0, 0)
    for skew in ((0, 0), (4, 0), (0, 2), (4, 2), (8, 4), (12, 6), (0, 8)):
        same_words(f"{dims} skew {skew}", device_distance(inst, spec_of(dims), words, 1, 9, 0, 0, f"{dims} skew {skew}", skew=skew), want)


def test_the_result_depends_on_nothing_but_the_volume_and_the_spec(inst):
    dims = (72, 40, 33)
    v, words = spec_of(dims), tier_words((72, 40, 33), 21, 0.002)
    first = device_distance(inst, v, words, 1, 12, 0, 0, "first")
    same_words("against the restatement", first, DR.distance(words, 1, 12, 0, 0))
    assert device_distance(inst, v, words, 1, 12, 0, 0, "second").tobytes() == first.tobytes()
    assert device_distance(inst, v, words, 1, 12, 0, 0, "zero-filled", fill=0x00).tobytes() == first.tobytes()
    # radius 3 after radius 255 into the same array equals a fresh call
    out = Off(2 * words.size)
    device_distance(inst, v, words, 1, 255, 0, 0, "r=255", out=out)
    again = device_distance(inst, v, words, 1, 3, 0, 0, "r=3 after r=255", out=out)
    fresh = device_distance(inst, v, words, 1, 3, 0, 0, "r=3")
    assert again.tobytes() == fresh.tobytes() and (fresh != FAR).sum() < (first != FAR).sum()
    same_words("r=3", fresh, DR.distance(words, 1, 3, 0, 0))


# ---- 4. the field --------------------------------------------------------------------------------------------------------------

def device_field(inst, v, o, i, label, skew=(0, 0, 0)):
    import torch
    d_o, d_i = Off(o.nbytes, o, off=skew[0]), (Off(i.nbytes, i, off=skew[1]) if i is not None else None)
    out = Off(4 * o.size, off=skew[2])
    torch.cuda.synchronize()
    assert inst.volume_distance_field(c_volume(v), d_o.ptr, d_i.ptr if i is not None else None, out.ptr) and inst.synchronize(), label
    assert d_o.read(label + " side 0").tobytes() == o.tobytes() and (i is None or d_i.read(label + " side 1").tobytes() == i.tobytes())
    return out.read(label, np.float32).reshape(o.shape).copy()


@pytest.mark.parametrize("nx", [36, 37])
def test_the_field_of_every_combination_of_words(inst, nx):
    """o and i words 0, 1, 2, 65025 and FAR in every combination and random ones, signed and unsigned, four voxels per lane
    (nx = 36) and one (nx = 37), and every array off its boundary in turn"""
    dims = (nx, 5, 3)
    rng = np.random.default_rng(nx)
    special = np.array([0, 1, 2, 65025, FAR], np.uint16)
    o = rng.integers(0, 65026, (3, 5, nx)).astype(np.uint16)
    i = rng.integers(0, 65026, (3, 5, nx)).astype(np.uint16)
    oo, ii = np.meshgrid(special, special, indexing="ij")
    o.reshape(-1)[:25], i.reshape(-1)[:25] = oo.reshape(-1), ii.reshape(-1)
    o.reshape(-1)[40:80] = 0
    for voxel in (0.0625, 0.05):
        v = spec_of(dims, voxel)
        for skew in ((0, 0, 0), (2, 0, 0), (0, 6, 0), (0, 0, 4), (8, 8, 8), (0, 0, 16)):
            got = device_field(inst, v, o, i, f"nx={nx} voxel={voxel} skew={skew}", skew)
            assert got.tobytes() == DR.field(o, i, voxel).tobytes(), (nx, voxel, skew)
            got = device_field(inst, v, o, None, f"nx={nx} voxel={voxel} skew={skew} unsigned", skew)
            assert got.tobytes() == DR.field(o, None, voxel).tobytes(), (nx, voxel, skew)


# ---- 5. scenes -----------------------------------------------------------------------------------------------------------------

def test_an_analytic_ball(inst):
    words, c = ball_scene()
    voxel, r, rho = 0.0625, 9, 6.0
    v = spec_of((32, 32, 32), voxel)
    o = device_distance(inst, v, words, 1, r, 0, 0, "outside")
    i = device_distance(inst, v, words, 1, r, 1, 0, "inside")
    f = device_field(inst, v, o, i, "field")
    assert f.tobytes() == DR.field(DR.distance(words, 1, r, 0, 0), DR.distance(words, 1, r, 1, 0), voxel).tobytes()
    check_ball(o, i, f, c, rho, r, voxel)


def test_a_fused_scene_both_sides_the_field_and_the_same_through_a_window(inst):
    """integrate on the device, then both sides, then the field, each against the restatement; then the same volume through
    sgm_volume_window with a margin of r voxels around a box: on the box, the source's distances word for word"""
    import torch
    v, s, poses, disp, words0, fused = fused_scene()
    maps = upload(disp)
    d_vox = Between(words0.nbytes, words0)
    torch.cuda.synchronize()
    assert inst.volume_integrate(c_volume(v), c_source(s), poses, maps.data_ptr(), None, None, d_vox.ptr) and inst.synchronize()
    shape = (v.nz, v.ny, v.nx)
    assert d_vox.read("fused").tobytes() == fused.tobytes()
    want_o, want_i, want_f, want_u = fused_reference()
    r = 6
    o = device_distance(inst, v, fused, 1, r, 0, 0, "side 0", d_vox=d_vox)
    i = device_distance(inst, v, fused, 1, r, 1, 0, "side 1", d_vox=d_vox)
    same_words("side 0", o, want_o)
    same_words("side 1", i, want_i)
    assert device_field(inst, v, o, i, "signed").tobytes() == want_f.tobytes() and device_field(inst, v, o, None, "unsigned").tobytes() == want_u.tobytes()
    assert d_vox.read("fused, afterwards").tobytes() == fused.tobytes()
    lo, n = (7, 6, 3), (6, 5, 4)
    offset, dims = tuple(c - r for c in lo), tuple(m + 2 * r for m in n)
    d_win = Between(4 * dims[0] * dims[1] * dims[2])
    w = inst.volume_window(c_volume(v), offset, dims, d_vox.ptr, None, d_win.ptr, None)
    assert w is not None and inst.synchronize()
    win = d_win.read("window", np.uint32).reshape(dims[2], dims[1], dims[0]).copy()
    assert win.tobytes() == WR.window(fused, v, offset, dims).tobytes()
    for side, whole in ((0, want_o), (1, want_i)):
        part = device_distance(inst, WR.window_spec(v, offset, dims), win, 1, r, side, 0, f"window side {side}", d_vox=d_win)
        same_words(f"window side {side}", part, DR.distance(win, 1, r, side, 0))
        box = whole[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]]
        assert np.array_equal(part[r:r + n[2], r:r + n[1], r:r + n[0]], box) and (box != FAR).any(), side
    assert maps.cpu().numpy().tobytes() == np.ascontiguousarray(disp).tobytes()


# ---- 6. refusals on the device build -------------------------------------------------------------------------------------------

def test_refusals_leave_the_poisoned_outputs_untouched(inst, capfd):
    import soc_project_stereo_matching_amd as S
    dims = (12, 6, 5)
    v, words = spec_of(dims), tier_words((12, 6, 5), 3, 0.1)
    n = words.size
    d_vox, d_out, d_in, d_field = Between(4 * n, words), Between(2 * n), Between(2 * n), Between(4 * n)
    ok = S.distance_spec(1, 3)
    bad_spec = c_volume(VR.spec(0, 6, 5, 0.0625, (0, 0, 0), 0.25))
    refusals = [
        lambda: inst.volume_distance(bad_spec, ok, d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), ok, None, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), ok, d_vox.ptr, None),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(0, 3), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(65536, 3), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(1, 0), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(1, 256), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(1, 3, 2, 0), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), S.distance_spec(1, 3, 0, -1), d_vox.ptr, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), ok, d_vox.ptr + 2, d_out.ptr),
        lambda: inst.volume_distance(c_volume(v), ok, d_vox.ptr, d_out.ptr + 1),
        lambda: inst.volume_distance(c_volume(v), ok, d_vox.ptr, d_vox.ptr + 4 * n - 2),
        lambda: inst.volume_distance_field(bad_spec, d_out.ptr, d_in.ptr, d_field.ptr),
        lambda: inst.volume_distance_field(c_volume(v), None, d_in.ptr, d_field.ptr),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr, d_in.ptr, None),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr + 1, None, d_field.ptr),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr, d_in.ptr + 1, d_field.ptr),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr, d_in.ptr, d_field.ptr + 2),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr, d_in.ptr, d_out.ptr),
        lambda: inst.volume_distance_field(c_volume(v), d_out.ptr, d_field.ptr + 4 * n - 2, d_field.ptr),
    ]
    for k, call in enumerate(refusals):
        capfd.readouterr()
        assert not call(), k
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("sgm_mi355x: sgm_volume_distance"), (k, err)
    assert inst.synchronize()
    for name, b in (("out", d_out), ("in", d_in), ("field", d_field)):
        assert np.all(b.read(name) == 0xA5), name
    assert d_vox.read("volume").tobytes() == words.tobytes()
