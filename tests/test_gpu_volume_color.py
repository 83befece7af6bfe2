"""Colour in the TSDF volume on the device (extension; include/sgm_mi355x.h, the colour section) against the numpy restatement
tests/color_ref.py -- needs an MI355X.  Tolerance 0 everywhere: words and bytes are compared.  Every array a call may write sits
between margins of 0xA5 (outputs are pre-filled with it), which are checked afterwards, and every coloured call is held against its
plain twin on the device: the TSDF words, the depth and the normals are the twin's, byte for byte."""
import numpy as np
import pytest

import cloud_ref as CR
import color_ref as KR
import mesh_ref as MR
import raycast_ref as RR
import volume_ref as VR
from conftest import load_npz
from test_color_cpu import colored_scene, images_of, invalid_ids, planted_start, slab_zeroed
from test_gpu_raycast import Between
from test_gpu_volume import c_source, c_volume, same_volume, side_maps, upload, volume
from test_raycast_cpu import c_view, same_maps, scene_view
from test_volume_cpu import camera, moving_rig, noisy_maps

pytestmark = pytest.mark.gpu

A5 = 0xA5A5A5A5


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: explicit maps need no shape
    yield i
    i.close()


# ---- integration ---------------------------------------------------------------------------------------------------------------

def fuse(inst, v, s, poses, disp, mask, conf, image, channels, vox0, col0, label, skew_vox=False, skew_col=False, skew_maps=False,
         twin=True):
    """one coloured call on the device: (voxels, colours) [nz][ny][nx]; the margins of both arrays whole, the inputs only read, and
    the voxels equal to what the plain call makes of a copy"""
    import torch
    d_vox, d_col = Between(vox0.nbytes, vox0, skew_vox), Between(col0.nbytes, col0, skew_col)
    maps = [upload(m, skew_maps) for m in (disp, mask, conf, image)]
    torch.cuda.synchronize()
    args = [None if m is None else m.data_ptr() for m in maps]
    assert inst.volume_integrate_color(c_volume(v), c_source(s), poses, args[0], args[1], args[2], args[3], channels, d_vox.ptr, d_col.ptr), label
    assert inst.synchronize(), label
    shape = (v.nz, v.ny, v.nx)
    vox, col = d_vox.read(label + " voxels", np.uint32).reshape(shape), d_col.read(label + " colours", np.uint32).reshape(shape)
    for m, host in zip(maps, (disp, mask, conf, image)):
        assert m is None or m.cpu().numpy().tobytes() == np.ascontiguousarray(host).tobytes(), f"{label}: an input changed"
    if twin:
        d_plain = Between(vox0.nbytes, vox0, skew_vox)
        torch.cuda.synchronize()
        assert inst.volume_integrate(c_volume(v), c_source(s), poses, args[0], args[1], args[2], d_plain.ptr) and inst.synchronize(), label
        same_volume(label + " against the plain call", vox, d_plain.read(label + " plain", np.uint32).reshape(shape))
    return vox, col


def check_fuse(inst, v, s, poses, disp, mask, conf, image, channels, vox0, col0, label, **kw):
    vox, col = fuse(inst, v, s, poses, disp, mask, conf, image, channels, vox0, col0, label, **kw)
    want_vox, want_col, stats = KR.integrate(vox0, col0, v, s, poses, disp, mask, conf, image, channels)
    same_volume(label + " voxels", vox, want_vox)
    same_volume(label + " colours", col, want_col)
    return want_vox, want_col, stats


@pytest.mark.parametrize("dims", [(8, 5, 3), (36, 33, 20), (37, 21, 5)])
def test_every_path_under_both_sources_and_both_image_kinds(inst, dims):
    for k, (w, h, frames) in enumerate(((24, 16, 1), (70, 33, 3))):
        for channels in (1, 4):
            for max_weight in (3, 1000):                          # the colour weight capped by max_weight, and by 255
                v = volume(dims, max_weight=max_weight)
                s = camera(w, h, frames=frames, min_conf=9)
                rng = np.random.default_rng(1000 * k + 10 * dims[0] + channels)
                disp = noisy_maps(s, rng)
                mask, conf = side_maps(s, rng)
                image = images_of(s, rng, channels)
                vox0, col0 = planted_start(v, rng)
                for sides in (False, True):
                    label = f"{dims} under {w}x{h}x{frames} channels={channels} max_weight={max_weight} maps={sides}"
                    _, col, stats = check_fuse(inst, v, s, moving_rig(frames), disp, mask if sides else None, conf if sides else None, image,
                                               channels, vox0, col0, label)
                    if not sides:                                 # the case is about something
                        assert stats["colored"] > 0.05 * frames * v.nx * v.ny * v.nz and stats["updates"] > stats["colored"], (label, stats)
                        assert stats["halves"] > 0, (label, stats)
                        top = KR.unpack(col)[3][col != col0].max()            # of the words that were painted
                        assert top <= min(max_weight, 255) and (top == min(max_weight, 255) or dims == (8, 5, 3)), (label, top)


def test_mixed_alignment_and_maps_one_element_off(inst):
    """one of the two arrays 4 bytes off a 16-byte boundary: one voxel per lane although nx % 4 == 0; both off; the maps off"""
    v = volume((36, 33, 20), max_weight=4)
    s = camera(70, 33, frames=3, min_conf=9)
    rng = np.random.default_rng(77)
    disp = noisy_maps(s, rng)
    mask, conf = side_maps(s, rng)
    vox0, col0 = planted_start(v, rng)
    for channels in (1, 4):
        image = images_of(s, rng, channels)
        for skew_vox, skew_col, skew_maps in ((False, True, False), (True, False, False), (True, True, False), (False, False, True), (True, True, True)):
            check_fuse(inst, v, s, moving_rig(3), disp, mask, conf, image, channels, vox0, col0,
                       f"channels={channels} voxels off={skew_vox} colours off={skew_col} maps off={skew_maps}", skew_vox=skew_vox,
                       skew_col=skew_col, skew_maps=skew_maps)


def test_the_scene_of_the_cpu_tests_meets_every_condition(inst):
    v, s, poses, disp, image, vox0, col0 = colored_scene()
    vox, col, stats = check_fuse(inst, v, s, poses, disp, None, None, image, 4, vox0, col0, "the coloured scene")
    w, cw = VR.unpack(vox)[1], KR.unpack(col)[3]
    assert ((w > 0) & (cw == 0)).sum() > 100 and stats["halves"] > 0 and cw.max() == 255


def test_batch_of_three_equals_three_calls_and_runs_repeat(inst):
    v, s, poses, disp, image, vox0, col0 = colored_scene()
    runs = [fuse(inst, v, s, poses, disp, None, None, image, 4, vox0, col0, "batch", twin=False) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    vox, col = vox0, col0
    for f in range(s.frames):
        s1 = CR.spec(s.width, s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, frames=1)
        vox, col = fuse(inst, v, s1, poses[f:f + 1], disp[f:f + 1], None, None, image[f:f + 1], 4, vox, col, f"frame {f}", twin=False)
    assert vox.tobytes() == runs[0][0].tobytes() and col.tobytes() == runs[0][1].tobytes()


def test_last_match_map_behind_a_match():
    """d_disp == NULL: the instance's last final map, coloured with the left image of the pair that was matched"""
    import torch
    import soc_project_stereo_matching_amd as S
    z = load_npz("tiny_t70x33_d16.npz")
    left, right = z["left"], z["right"]
    h, w = left.shape
    s = CR.spec(w, h, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=0.25)
    v = VR.spec(36, 33, 20, 0.1, (-1.8, -1.65, 0.5), 0.4)
    i = S.SGMInstance(0)
    try:
        for overlap in (False, True):
            assert i.set_overlap_post(overlap) and i.reset(w, h, S.default_option(16, min_speckle_area=9))
            d_vox, d_col = Between(4 * v.nx * v.ny * v.nz, VR.empty(v)), Between(4 * v.nx * v.ny * v.nz, KR.empty(v))
            d_img = torch.from_numpy(left).cuda()
            torch.cuda.synchronize()
            assert i.match(left, right) is not None
            assert i.volume_integrate_color(c_volume(v), c_source(s), VR.pose(), None, None, None, d_img.data_ptr(), 1, d_vox.ptr, d_col.ptr)
            assert i.synchronize()
            final = i.read_stage("final")
            want_vox, want_col, stats = KR.integrate(VR.empty(v), KR.empty(v), v, s, VR.pose()[None], final.reshape(1, h, w), None, None,
                                                     left.reshape(1, h, w), 1)
            assert stats["colored"] > 300, stats
            same_volume(f"overlap={overlap} voxels", d_vox.read("voxels", np.uint32).reshape(want_vox.shape), want_vox)
            same_volume(f"overlap={overlap} colours", d_col.read("colours", np.uint32).reshape(want_col.shape), want_col)
    finally:
        i.close()


# ---- ray-cast ------------------------------------------------------------------------------------------------------------------

_painted = {}


def painted(dims):
    """(v, voxels, colours) of the volume `dims` after three noisy coloured frames, by the restatement; computed once"""
    if dims not in _painted:
        v = volume(dims, max_weight=5)
        s = camera(70, 33, frames=3)
        rng = np.random.default_rng(161 + dims[0])
        vox, col, _ = KR.integrate(VR.empty(v), KR.empty(v), v, s, moving_rig(3), noisy_maps(s, rng), None, None, images_of(s, rng, 4), 4)
        if min(dims) > 1:
            col = slab_zeroed(v, col)
        vox.setflags(write=False)
        col.setflags(write=False)
        _painted[dims] = (v, vox, col)
    return _painted[dims]


def render(inst, v, vox, col, vw, poses, label, normals=True, skew=False):
    """one coloured call: (depth, normal or None, rgba); margins whole, the volume and the colours only read, depth and normals the
    bytes of the plain call"""
    import torch
    px = vw.frames * vw.height * vw.width
    d_vox, d_col = Between(vox.nbytes, vox, skew), Between(col.nbytes, col, skew)
    outs = [Between(4 * px, skew=skew), Between(12 * px, skew=skew), Between(4 * px, skew=skew)]
    plain = [Between(4 * px, skew=skew), Between(12 * px, skew=skew)]
    torch.cuda.synchronize()
    assert inst.volume_raycast_color(c_volume(v), c_view(vw), poses, d_vox.ptr, d_col.ptr, outs[0].ptr, outs[1].ptr if normals else None,
                                     outs[2].ptr), label
    assert inst.volume_raycast(c_volume(v), c_view(vw), poses, d_vox.ptr, plain[0].ptr, plain[1].ptr if normals else None), label
    assert inst.synchronize(), label
    shape = (vw.frames, vw.height, vw.width)
    depth, normal = outs[0].read(label + " depth", np.uint32), outs[1].read(label + " normal", np.uint32)
    rgba = outs[2].read(label + " rgba", np.uint32).reshape(shape)
    assert depth.tobytes() == plain[0].read(label, np.uint32).tobytes(), f"{label}: the depth is not the plain call's"
    assert normal.tobytes() == plain[1].read(label, np.uint32).tobytes(), f"{label}: the normals are not the plain call's"
    assert d_vox.read(label).tobytes() == np.ascontiguousarray(vox).tobytes() and d_col.read(label).tobytes() == np.ascontiguousarray(col).tobytes()
    if not normals:
        assert np.all(normal == A5), f"{label}: wrote normals that were not asked for"
    return depth.view(np.float32).reshape(shape), normal.view(np.float32).reshape(shape + (3,)) if normals else None, rgba


def check_render(inst, v, vox, col, vw, poses, label, **kw):
    depth, normal, rgba = render(inst, v, vox, col, vw, poses, label, **kw)
    want_d, want_n, want_c, stats = KR.raycast(vox, col, v, vw, poses)
    same_maps(label + " depth", depth, want_d)
    if normal is not None:
        same_maps(label + " normal", normal, want_n)
    if not np.array_equal(rgba, want_c):
        bad = np.argwhere(rgba != want_c)
        raise AssertionError(f"{label}: {len(bad)} of {rgba.size} colours differ, first at {tuple(bad[0])}: {rgba[tuple(bad[0])]:#010x} != "
                             f"{want_c[tuple(bad[0])]:#010x}")
    return stats


def test_every_view_with_and_without_normals_meets_all_four_pixel_classes(inst):
    v, vox, col = painted((36, 33, 20))
    total = dict(trilinear=0, nearest=0, uncolored=0, empty=0)
    for k, (w, h) in enumerate(((24, 16), (70, 33), (33, 9))):
        frames = (1, 3)[k % 2]
        for kw in (dict(), dict(normals=False), dict(skew=True)):
            stats = check_render(inst, v, vox, col, scene_view(w, h, frames=frames), moving_rig(frames), f"{w}x{h}x{frames} {kw}", **kw)
        for name in total:
            total[name] += stats[name]
    assert min(total.values()) > 0 and total["trilinear"] > 500, total


@pytest.mark.parametrize("dims", [(1024, 1, 1), (1, 1024, 1), (1, 1, 1024), (37, 21, 5), (8, 5, 3)])
def test_the_degenerate_and_the_odd_volumes(inst, dims):
    v, vox, col = painted(dims)
    needle = dims == (1, 1, 1024)
    vw = scene_view(33, 9, frames=2, z_min=0.9 if needle else 0.3, z_max=1.2 if needle else 1.6, step=0.004 if needle else 0.1)
    check_render(inst, v, vox, col, vw, moving_rig(2), f"{dims}")


def test_64_frames(inst):
    v, vox, col = painted((36, 33, 20))
    stats = check_render(inst, v, vox, col, scene_view(24, 16, frames=64), moving_rig(64), "64 frames")
    assert stats["trilinear"] > 64 * 50


# ---- the colours of a list -----------------------------------------------------------------------------------------------------

def colours_of(inst, v, vox, col, records, id_kinds, label, count="none", capacity=None, skew=False):
    """one call on uploaded records: the uint32 written for the records handled; everything else still 0xA5.  count: "none" (NULL)
    or the number a device word holds"""
    import torch
    capacity = len(records) if capacity is None else capacity
    d_vox, d_col = Between(vox.nbytes, vox, skew), Between(col.nbytes, col, skew)
    d_rec = torch.full((16 * (max(len(records), capacity) + 2),), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_rec.data_ptr() % 16 == 0
    r_off = 16 if skew else 0
    if len(records):
        d_rec[r_off:r_off + 16 * len(records)].copy_(torch.from_numpy(np.ascontiguousarray(records).view(np.uint8)))
    d_cnt = Between(4, np.array([0 if count == "none" else count], np.uint32), skew)
    d_out = Between(4 * capacity, skew=skew)
    torch.cuda.synchronize()
    assert inst.volume_colors(c_volume(v), d_vox.ptr, d_col.ptr, d_rec.data_ptr() + r_off if capacity else None, capacity,
                              None if count == "none" else d_cnt.ptr, id_kinds, d_out.ptr if capacity else None), label
    assert inst.synchronize(), label
    handled = capacity if count == "none" else min(capacity, count)
    out = d_out.read(label, np.uint32)
    assert np.all(out[handled:] == A5), f"{label}: records beyond the count were written"
    assert d_vox.read(label).tobytes() == np.ascontiguousarray(vox).tobytes() and d_col.read(label).tobytes() == np.ascontiguousarray(col).tobytes()
    d_cnt.read(label)
    return out[:handled]


def same_colours(label, got, want):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{label}: {len(bad)} of {len(want)} colours differ, first at {bad[0]}: {got[bad[0]]:#010x} != {want[bad[0]]:#010x}")


def test_vertices_and_points_of_an_integrated_scene_and_of_a_sphere(inst):
    rng = np.random.default_rng(5)
    v, vox, col = painted((36, 33, 20))
    sv, svox = MR.sphere((19, 14, 11))
    scol = rng.integers(0, 1 << 32, svox.shape, dtype=np.uint64).astype(np.uint32)
    scol[rng.random(svox.shape) < 0.3] &= np.uint32(0x00FFFFFF)                  # three in ten voxels without colour
    for name, (a, b, c) in (("scene", (v, vox, col)), ("sphere", (sv, svox, scol))):
        classes = set()
        for kinds, recs in ((8, MR.vertices(b, a, 1)), (4, VR.crossings(b, a, 1))):
            assert len(recs) > 257
            want = KR.colors(b, c, a, recs["id"], kinds)
            classes |= set(KR.color_classes(b, c, a, recs["id"], kinds).tolist())
            for skew in (False, True):
                same_colours(f"{name} kinds={kinds} skew={skew}", colours_of(inst, a, b, c, recs, kinds, f"{name} {kinds}", skew=skew), want)
            for count in (0, 1, 257):                             # nothing; one lane; two workgroups, the second with one lane
                same_colours(f"{name} kinds={kinds} count={count}", colours_of(inst, a, b, c, recs, kinds, f"{name} {kinds} count {count}", count=count),
                             want[:count])
            same_colours(f"{name} kinds={kinds} count above the capacity",
                         colours_of(inst, a, b, c, recs, kinds, f"{name} {kinds} capacity 100", count=len(recs), capacity=100), want[:100])
        assert classes >= {1, 2, 3} if name == "sphere" else 3 in classes, (name, classes)


def test_planted_invalid_ids(inst):
    v, vox, col = painted((36, 33, 20))
    for kinds in (4, 8):
        ids = invalid_ids(v, kinds)
        recs = np.zeros(len(ids), MR.VERTEX)
        recs["x"] = np.float32("nan")                             # only the id is read
        recs["id"] = ids
        want = KR.colors(vox, col, v, ids, kinds)
        assert set(KR.color_classes(vox, col, v, ids, kinds).tolist()) >= {0, 3} and (want == 0).sum() >= 4
        same_colours(f"invalid ids, kinds={kinds}", colours_of(inst, v, vox, col, recs, kinds, f"invalid {kinds}"), want)


def test_queued_behind_the_mesh_and_the_points_with_their_counts(inst):
    """mesh (or points), then the colours with the list's own count word, no wait in between; the capacity is above the count"""
    import torch
    v, vox, col = painted((36, 33, 20))
    d_vox, d_col = Between(vox.nbytes, vox), Between(col.nbytes, col)
    for kinds, want_recs in ((8, MR.vertices(vox, v, 1)), (4, VR.crossings(vox, v, 1))):
        cap = len(want_recs) + 300
        d_rec = torch.full((16 * cap,), 0xA5, dtype=torch.uint8, device="cuda")
        d_tri = torch.full((16 * 12 * vox.size // 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_cnt, d_out = Between(8), Between(4 * cap)
        torch.cuda.synchronize()
        if kinds == 8:
            assert inst.volume_mesh(c_volume(v), d_vox.ptr, 1, d_rec.data_ptr(), cap, d_tri.data_ptr(), d_tri.numel() // 16, d_cnt.ptr)
        else:
            assert inst.volume_points(c_volume(v), d_vox.ptr, 1, d_rec.data_ptr(), cap, d_cnt.ptr)
        assert inst.volume_colors(c_volume(v), d_vox.ptr, d_col.ptr, d_rec.data_ptr(), cap, d_cnt.ptr, kinds, d_out.ptr)
        assert inst.synchronize()
        count = int(d_cnt.read("count", np.uint32)[0])
        assert count == len(want_recs) < cap
        assert d_rec.cpu().numpy()[:16 * count].tobytes() == want_recs.tobytes()
        out = d_out.read("colours", np.uint32)
        same_colours(f"queued, kinds={kinds}", out[:count], KR.colors(vox, col, v, want_recs["id"], kinds))
        assert np.all(out[count:] == A5)


# ---- general -------------------------------------------------------------------------------------------------------------------

def test_every_refusal_queues_nothing(inst):
    import torch
    v, s, poses, disp, image, vox0, col0 = colored_scene()
    n = v.nx * v.ny * v.nz
    d_vox, d_col = Between(4 * n, np.full(n, A5, np.uint32)), Between(4 * n, np.full(n, A5, np.uint32))
    d, img = upload(disp), upload(image)
    vw = scene_view(24, 16)
    px = 24 * 16
    d_depth, d_normal, d_rgba = Between(4 * px), Between(12 * px), Between(4 * px)
    d_rec, d_cnt, d_out = Between(16 * 64), Between(4), Between(4 * 64)
    cv, cs, cw = c_volume(v), c_source(s), c_view(vw)
    x, c, m, g = d_vox.ptr, d_col.ptr, d.data_ptr(), img.data_ptr()
    zd, zn, zc = d_depth.ptr, d_normal.ptr, d_rgba.ptr
    r, k, o = d_rec.ptr, d_cnt.ptr, d_out.ptr
    one = VR.pose()[None]
    nan = float("nan")
    bad_v = c_volume(v)
    bad_v.nx = 1025
    bad_s = c_source(s)
    bad_s.fx = nan
    bad_w = c_view(vw)
    bad_w.step = 0.0
    bad_pose = poses.copy()
    bad_pose[1, 3] = nan
    fuse_ = lambda *a: inst.volume_integrate_color(*a)
    for t, args in enumerate((
            (bad_v, cs, poses, m, None, None, g, 4, x, c), (cv, bad_s, poses, m, None, None, g, 4, x, c), (cv, cs, bad_pose, m, None, None, g, 4, x, c),
            (cv, cs, poses, None, None, None, g, 4, x, c),                                    # no match to take a map from
            (cv, cs, poses, m, None, None, None, 4, x, c), (cv, cs, poses, m, None, None, g, 4, x, None),              # NULL image, colours
            (cv, cs, poses, m, None, None, g, 3, x, c), (cv, cs, poses, m, None, None, g, 0, x, c), (cv, cs, poses, m, None, None, g, 2, x, c),
            (cv, cs, poses, m, None, None, g + 2, 4, x, c), (cv, cs, poses, m, None, None, g, 4, x, c + 2), (cv, cs, poses, m, None, None, g, 4, x + 1, c),
            (cv, cs, poses, m, None, None, g, 4, x, x), (cv, cs, poses, m, None, None, g, 4, x, x + 4 * (n - 1)),      # colours over the volume
            (cv, cs, poses, m, None, None, g, 4, x, g), (cv, cs, poses, m, None, None, g, 4, x, m), (cv, cs, poses, m, c, None, g, 4, x, c))):
        assert not fuse_(*args), t
    for t, args in enumerate((
            (bad_v, cw, one, x, c, zd, zn, zc), (cv, bad_w, one, x, c, zd, zn, zc), (cv, cw, one * nan, x, c, zd, zn, zc),
            (cv, cw, one, None, c, zd, zn, zc), (cv, cw, one, x, None, zd, zn, zc), (cv, cw, one, x, c, None, zn, zc), (cv, cw, one, x, c, zd, zn, None),
            (cv, cw, one, x, c + 2, zd, zn, zc), (cv, cw, one, x, c, zd, zn, zc + 2), (cv, cw, one, x, c, zd + 1, zn, zc),
            (cv, cw, one, x, c, zd, zn, x), (cv, cw, one, x, c, zd, zn, c + 16), (cv, cw, one, x, c, zd, zn, zd), (cv, cw, one, x, c, zd, zn, zn + 8),
            (cv, cw, one, x, c, c, zn, zc))):
        assert not inst.volume_raycast_color(*args), t
    big = c_volume(VR.spec(1024, 1024, 256, 0.01, (0, 0, 0), 0.1))                           # 2^28 voxels: too many for mesh ids
    for t, args in enumerate((
            (bad_v, x, c, r, 64, k, 8, o), (cv, None, c, r, 64, k, 8, o), (cv, x, None, r, 64, k, 8, o), (cv, x, c, None, 64, k, 8, o),
            (cv, x, c, r, 64, k, 8, None), (cv, x, c, r, 64, k, 7, o), (cv, x, c, r, 64, k, 0, o), (big, x, c, r, 64, k, 8, o),
            (cv, x, c, r + 8, 63, k, 8, o), (cv, x + 2, c, r, 64, k, 8, o), (cv, x, c + 2, r, 64, k, 8, o), (cv, x, c, r, 64, k + 2, 8, o),
            (cv, x, c, r, 64, k, 8, o + 2), (cv, x, c, r, 64, k, 8, x), (cv, x, c, r, 64, k, 8, c), (cv, x, c, r, 64, k, 8, r), (cv, x, c, r, 64, o, 8, o))):
        assert not inst.volume_colors(*args), t
    assert inst.volume_colors(cv, x, c, None, 0, None, 8, None)                              # capacity 0: a successful no-op
    assert inst.synchronize()
    torch.cuda.synchronize()
    for b in (d_vox, d_col, d_depth, d_normal, d_rgba, d_rec, d_cnt, d_out):
        assert bool((b.hold == 0xA5).all())
    assert d.cpu().numpy().tobytes() == disp.tobytes() and img.cpu().numpy().tobytes() == image.tobytes()
    # the instance still works
    vox, col, _ = check_fuse(inst, v, s, poses, disp, None, None, image, 4, vox0, col0, "after the refusals")
    assert check_render(inst, v, vox, col, vw, one, "after the refusals")["trilinear"] > 50


def one_round(inst, dims, source, seed, label):
    """integrate, render, mesh colours: the three calls on one volume against the restatement"""
    w, h, frames = source
    v = volume(dims, max_weight=5)
    s = camera(w, h, frames=frames)
    rng = np.random.default_rng(seed)
    vox0, col0 = planted_start(v, rng)
    vox, col, _ = check_fuse(inst, v, s, moving_rig(frames), noisy_maps(s, rng), None, None, images_of(s, rng, 1), 1, vox0, col0, label)
    stats = check_render(inst, v, vox, col, scene_view(33, 9), VR.pose()[None], label)
    recs = MR.vertices(vox, v, 1)
    same_colours(label, colours_of(inst, v, vox, col, recs, 8, label), KR.colors(vox, col, v, recs["id"], 8))
    return stats


def test_one_instance_through_a_large_volume_a_small_one_and_a_large_one_again():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    try:
        for k, (dims, source) in enumerate((((36, 33, 20), (70, 33, 3)), ((8, 5, 3), (24, 16, 1)), ((36, 33, 20), (24, 16, 2)))):
            one_round(i, dims, source, 300 + k, f"step {k}: {dims}")
    finally:
        i.close()


def test_under_guard_bands(monkeypatch):
    """the debug allocation mode of the instance: the three calls allocate nothing, and the bands of what the instance holds stay whole"""
    import torch
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(1 << 20))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    i = S.SGMInstance(0)
    try:
        assert one_round(i, (36, 33, 20), (70, 33, 3), 400, "guarded")["trilinear"] > 10
        torch.cuda.synchronize()
        assert S.debug_guard_check()[0] == 0
    finally:
        i.close()
    assert S.debug_guard_check() == (0, 0, 0)
