"""The TSDF volume ray-cast into depth and normal maps on the device (extension; include/sgm_mi355x.h, sgm_raycast_spec) against the
numpy restatement tests/raycast_ref.py -- needs an MI355X.  Tolerance 0 everywhere: maps are compared bit by bit.  The volumes are
filled by the restatement's integrate or planted, and uploaded (the integration kernel is not involved, except where the test is
about the queue); the outputs sit between margins of 0xA5, which are checked afterwards, as is the volume."""
import numpy as np
import pytest

import cloud_ref as CR
import raycast_ref as RR
import volume_ref as VR
from conftest import load_npz
from test_gpu_volume import c_source, c_volume, volume
from test_raycast_cpu import PLANTED_RAYS, c_view, noisy_poses, noisy_volume, plane_volume, same_maps, scene_view
from test_volume_cpu import camera, moving_rig, noisy_maps, rot

pytestmark = pytest.mark.gpu

MARGIN = 64                                                       # bytes of 0xA5 on either side of a buffer
VIEWS = [(70, 33), (24, 16), (1, 1), (65, 3), (3, 65), (129, 2)]  # 65 and 129: an edge in both directions for either wave mapping


class Between:
    """`nbytes` on the device between two margins of 0xA5, pre-filled with 0xA5 or with `data`; skew: one 4-byte element off a
    16-byte boundary"""
    def __init__(self, nbytes, data=None, skew=False):
        import torch
        self.torch, self.nbytes = torch, nbytes
        self.off = MARGIN + (4 if skew else 0)
        self.hold = torch.full((nbytes + 2 * MARGIN + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.hold.data_ptr() % 16 == 0
        if data is not None:
            self.hold[self.off:self.off + nbytes].copy_(torch.from_numpy(np.array(data).reshape(-1).view(np.uint8)))

    @property
    def ptr(self):
        return self.hold.data_ptr() + self.off

    def read(self, label, dtype=np.uint8):
        raw = self.hold.cpu().numpy()
        lo, hi = self.off, self.off + self.nbytes
        assert np.all(raw[:lo] == 0xA5) and np.all(raw[hi:] == 0xA5), f"{label}: wrote outside the buffer"
        return raw[lo:hi].view(dtype)


def render(inst, v, vox, vw, poses, label, normals=True, skew=False, skew_volume=False, volume_buf=None):
    """one call on the device: (depth, normal or None); the margins, the volume and, without normals, the normals' place untouched"""
    import torch
    px = vw.frames * vw.height * vw.width
    d_vox = volume_buf or Between(vox.nbytes, vox, skew_volume)
    d_depth, d_normal = Between(4 * px, skew=skew), Between(12 * px, skew=skew)
    torch.cuda.synchronize()
    assert inst.volume_raycast(c_volume(v), c_view(vw), poses, d_vox.ptr, d_depth.ptr, d_normal.ptr if normals else None), label
    assert inst.synchronize(), label
    depth = d_depth.read(label + " depth", np.float32).reshape(vw.frames, vw.height, vw.width)
    normal = d_normal.read(label + " normal", np.float32).reshape(vw.frames, vw.height, vw.width, 3)
    if volume_buf is None:
        assert d_vox.read(label + " volume").tobytes() == np.ascontiguousarray(vox).tobytes(), f"{label}: the volume is only read"
    if not normals:
        assert np.all(normal.view(np.uint32) == 0xA5A5A5A5), f"{label}: wrote normals that were not asked for"
        return depth, None
    return depth, normal


def check(inst, v, vox, vw, poses, label, **kw):
    """one call against the restatement; returns the restatement's stats"""
    depth, normal = render(inst, v, vox, vw, poses, label, **kw)
    want_d, want_n, stats = RR.raycast(vox, v, vw, poses)
    same_maps(label + " depth", depth, want_d)
    if normal is not None:
        same_maps(label + " normal", normal, want_n)
    return stats


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: the ray-cast needs no shape
    yield i
    i.close()


_filled = {}


def filled(dims):
    """the volume `dims` of tests/test_gpu_volume.py after three noisy frames from the moving rig, by the restatement; computed once"""
    if dims not in _filled:
        v = volume(dims, max_weight=5)
        s = camera(70, 33, frames=3)
        vox = VR.integrate(VR.empty(v), v, s, moving_rig(3), noisy_maps(s, np.random.default_rng(61 + dims[0])))[0]
        vox.setflags(write=False)
        _filled[dims] = (v, vox)
    return _filled[dims]


def test_the_designs_scenes(inst):
    v, vox = plane_volume()
    for size, hits, failed, normals in (((70, 33), 1856, 322, 1728), ((24, 16), 220, 44, 220)):
        stats = check(inst, v, vox, scene_view(*size), VR.pose()[None], "plane %dx%d" % size)
        assert stats == dict(hits=hits, back=0, refine_failed=failed, normals=normals)
    v, vox = noisy_volume()
    stats = check(inst, v, vox, scene_view(40, 24, frames=3), noisy_poses(), "noisy")
    assert stats["hits"] > 1000 and stats["back"] >= 1 and stats["refine_failed"] >= 1 and stats["normals"] < stats["hits"]


@pytest.mark.parametrize("dims", [(36, 33, 20), (37, 21, 5), (8, 5, 3), (1, 1, 1024)])
def test_every_volume_under_every_view(inst, dims):
    v, vox = filled(dims)
    total = 0
    for k, (w, h) in enumerate(VIEWS):
        frames = (1, 3)[k % 2]
        step = 0.004 if dims == (1, 1, 1024) else 0.1             # the needle's voxels are 1 / 1024 deep
        vw = scene_view(w, h, frames=frames, z_min=0.9 if dims == (1, 1, 1024) else 0.3, z_max=1.2 if dims == (1, 1, 1024) else 1.6, step=step)
        total += check(inst, v, vox, vw, moving_rig(frames), f"{dims} under {w}x{h}x{frames}")["hits"]
    # the cases are about something, except the volumes with no cell to interpolate in (nz or nx, ny below 2 voxels of surface)
    assert total > 100 or dims in ((1, 1, 1024),), (dims, total)


def test_64_frames(inst):
    v, vox = noisy_volume()
    stats = check(inst, v, vox, scene_view(24, 16, frames=64), moving_rig(64), "64 frames")
    assert stats["hits"] > 64 * 100


CAMERAS = {
    # name: (pose, view keywords, what the restatement must say)
    "outside and looking in": (VR.pose(), {}, lambda st: st["hits"] > 1000),
    "inside the volume": (VR.pose(np.eye(3), (0.0, 0.0, -0.7)), dict(z_min=0.0, z_max=1.0, step=0.05), lambda st: st["hits"] > 1000),
    "outside and looking away": (VR.pose(rot(1, np.pi)), {}, lambda st: st["hits"] == st["back"] == st["refine_failed"] == 0),
    "behind the volume": (VR.pose(np.eye(3), (0.0, 0.0, -2.0)), dict(z_min=0.0), lambda st: st["hits"] == 0),
    "rotated, from the side": (VR.pose(rot(1, 0.2), (0.25, -0.05, 0.1)), {}, lambda st: st["hits"] > 500 and st["refine_failed"] > 0),
    "min_weight above every weight": (VR.pose(), dict(min_weight=3), lambda st: st["hits"] == st["back"] == st["refine_failed"] == 0),
    "z_max in front of the surface": (VR.pose(), dict(z_max=0.8), lambda st: st["hits"] == st["refine_failed"] == 0),
    "a step larger than trunc": (VR.pose(), dict(step=0.35), lambda st: True),
    "a step that samples every voxel thrice": (VR.pose(), dict(step=0.0166), lambda st: st["hits"] > 1000),
}


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_cameras(inst, name):
    v, vox = noisy_volume()                                       # weights up to 2
    pose, kw, expect = CAMERAS[name]
    stats = check(inst, v, vox, scene_view(70, 33, **kw), pose[None], name)
    assert expect(stats), stats


def test_rays_parallel_to_voxel_faces(inst):
    """cx, cy on a pixel: its ray has gd_x == gd_y == 0, and the rays of its row and column have one of them"""
    v, vox = plane_volume()
    vw = RR.view(9, 7, 40.0, 40.0, 4.0, 3.0, 0.3, 1.6, 0.1)
    stats = check(inst, v, vox, vw, VR.pose()[None], "parallel")
    assert stats["hits"] == 63
    # ... and on a face exactly: the volume's origin moved so that the central ray runs in the plane x = 18 of the grid
    shifted = VR.spec(v.nx, v.ny, v.nz, v.voxel, (-18 * np.float32(0.05), v.origin[1], v.origin[2]), v.trunc)
    check(inst, shifted, vox, vw, VR.pose()[None], "on a face")


def test_planted_rays(inst):
    for name, (make, _, _, _) in sorted(PLANTED_RAYS.items()):
        v, vox, vw, poses = make()
        check(inst, v, vox, vw, poses, name)


def test_without_normals_and_pointers_one_element_off(inst):
    v, vox = noisy_volume()
    for w, h in ((70, 33), (65, 3), (1, 1)):
        vw = scene_view(w, h, frames=3)
        for kw in (dict(normals=False), dict(skew=True), dict(skew=True, normals=False), dict(skew_volume=True), dict(skew=True, skew_volume=True)):
            check(inst, v, vox, vw, noisy_poses(), f"{w}x{h} {kw}", **kw)


def test_batch_equals_frame_by_frame_and_runs_repeat(inst):
    v, vox = noisy_volume()
    vw, poses = scene_view(40, 24, frames=3), noisy_poses()
    runs = [render(inst, v, vox, vw, poses, "batch") for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    for f in range(3):
        d, n = render(inst, v, vox, scene_view(40, 24), poses[f:f + 1], f"frame {f}")
        assert d.tobytes() == runs[0][0][f].tobytes() and n.tobytes() == runs[0][1][f].tobytes(), f


def test_two_calls_behind_a_match_and_an_integration_see_the_integrated_volume():
    """match, integrate the instance's own map, render twice, all queued without a wait in between, with and without the post pass on
    a stream of its own: the renders equal the restatement of integrate, then raycast"""
    import torch
    import soc_project_stereo_matching_amd as S
    z = load_npz("tiny_t70x33_d16.npz")
    left, right = z["left"], z["right"]
    h, w = left.shape
    s = CR.spec(w, h, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=0.25)         # fb = 10: disparities 0.6..10 are depths 1..16
    v = VR.spec(36, 33, 20, 0.1, (-1.8, -1.65, 0.5), 0.4)
    views = [RR.view(w, h, 40.0, 40.0, 34.5, 16.0, 0.4, 2.6, 0.15), RR.view(33, 20, 20.0, 20.0, 16.0, 9.5, 0.4, 2.6, 0.1, frames=2)]
    poses = [VR.pose()[None], moving_rig(2)]
    i = S.SGMInstance(0)
    try:
        for overlap in (False, True):
            assert i.set_overlap_post(overlap) and i.reset(w, h, S.default_option(16, min_speckle_area=9))
            d_vox = Between(4 * v.nx * v.ny * v.nz, np.zeros(v.nx * v.ny * v.nz, np.uint32))
            outs = [(Between(4 * t.frames * t.height * t.width), Between(12 * t.frames * t.height * t.width)) for t in views]
            torch.cuda.synchronize()
            assert i.match(left, right) is not None
            d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            d_out = torch.empty((h, w), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert i.match_device(d_l.data_ptr(), d_r.data_ptr(), d_out.data_ptr())
            assert i.volume_integrate(c_volume(v), c_source(s), VR.pose(), d_out.data_ptr(), None, None, d_vox.ptr)
            for t, p, (dd, dn) in zip(views, poses, outs):
                assert i.volume_raycast(c_volume(v), c_view(t), p, d_vox.ptr, dd.ptr, dn.ptr)
            assert i.synchronize()
            disp = d_out.cpu().numpy()
            want_vox, updates = VR.integrate(VR.empty(v), v, s, VR.pose()[None], disp.reshape(1, h, w))
            assert updates > 500
            assert d_vox.read("volume", np.uint32).tobytes() == want_vox.tobytes()
            for k, (t, p, (dd, dn)) in enumerate(zip(views, poses, outs)):
                want_d, want_n, stats = RR.raycast(want_vox, v, t, p)
                assert stats["hits"] > 50, (k, stats)
                same_maps(f"overlap={overlap} call {k} depth", dd.read("depth", np.float32), want_d)
                same_maps(f"overlap={overlap} call {k} normal", dn.read("normal", np.float32), want_n)
    finally:
        i.close()


def test_every_refusal_queues_nothing(inst):
    import torch
    v, vox = noisy_volume()
    vw = scene_view(24, 16)
    d_vox = Between(vox.nbytes, np.full(vox.size, 0xA5A5A5A5, np.uint32))
    d_depth, d_normal = Between(4 * 24 * 16), Between(12 * 24 * 16)
    cv, cw, poses = c_volume(v), c_view(vw), VR.pose()[None]
    x, d, n = d_vox.ptr, d_depth.ptr, d_normal.ptr
    nan = float("nan")

    def view(**kw):
        t = c_view(vw)
        for name, val in kw.items():
            setattr(t, name, val)
        return t

    for k, t in enumerate((view(width=0), view(height=65536), view(frames=0), view(frames=65), view(fx=0.0), view(fy=nan), view(cx=float("inf")),
                           view(z_min=-1.0), view(z_max=float("inf")), view(z_max=0.2), view(step=0.0), view(step=1e-6), view(min_weight=0),
                           view(min_weight=65536))):
        assert not inst.volume_raycast(cv, t, moving_rig(65)[:t.frames], x, d, n), k
    bad_volume = c_volume(v)
    bad_volume.nx = 1025
    bad_pose = poses.copy()
    bad_pose[0, 10] = nan
    assert not inst.volume_raycast(bad_volume, cw, poses, x, d, n) and not inst.volume_raycast(cv, cw, bad_pose, x, d, n)
    assert not inst.volume_raycast(cv, cw, poses, x + 2, d, n) and not inst.volume_raycast(cv, cw, poses, x, d + 2, n)
    assert not inst.volume_raycast(cv, cw, poses, x, d, n + 1)
    assert not inst.volume_raycast(cv, cw, poses, x, x + 16, n) and not inst.volume_raycast(cv, cw, poses, x, d, x) and not inst.volume_raycast(cv, cw, poses, x, d, d)
    assert not inst.volume_raycast(cv, cw, poses, None, d, n) and not inst.volume_raycast(cv, cw, poses, x, None, n)
    assert inst.synchronize()
    torch.cuda.synchronize()
    for b in (d_vox, d_depth, d_normal):
        assert bool((b.hold == 0xA5).all())


def test_under_guard_bands(monkeypatch):
    """the debug allocation mode of the instance: the ray-cast allocates nothing, and the bands of what the instance holds stay whole"""
    import torch
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(1 << 20))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    i = S.SGMInstance(0)
    try:
        v, vox = noisy_volume()
        check(i, v, vox, scene_view(70, 33, frames=3), noisy_poses(), "guarded")
        torch.cuda.synchronize()
        assert S.debug_guard_check()[0] == 0
    finally:
        i.close()
    assert S.debug_guard_check() == (0, 0, 0)
