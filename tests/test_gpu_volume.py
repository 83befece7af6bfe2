"""Depth fused into a TSDF volume on the device (extension; include/sgm_mi355x.h, sgm_volume_spec) against the numpy restatement
tests/volume_ref.py -- needs an MI355X.  Tolerance 0 everywhere: volumes are compared word by word, surface lists byte by byte, the
buffers are pre-filled with 0xA5 around (and, for the list, inside) what a call may write, and what must not be written is checked."""
import numpy as np
import pytest

import cloud_ref as CR
import volume_ref as VR
from conftest import load_npz
from test_volume_cpu import PLANTED, camera, moving_rig, noisy_maps, noisy_scene, plane_scene, planted_crossings, planted_scene, rot

pytestmark = pytest.mark.gpu

MARGIN = 64                                                       # bytes of 0xA5 on either side of a volume


def c_volume(v):
    import soc_project_stereo_matching_amd as S
    return S.volume_spec(v.nx, v.ny, v.nz, v.voxel, v.origin, v.trunc, v.max_weight)


def c_source(s):
    import soc_project_stereo_matching_amd as S
    return S.SGMCloudSpec(s.width, s.height, s.frames, s.fx, s.fy, s.cx, s.cy, s.baseline, s.doffs, s.z_min, s.z_max, s.min_conf)


# the volumes of the tests, all around the surface near Z = 1.03 the scenes' cameras see: nx, ny, nz -> voxel, origin
VOLUMES = {
    (8, 5, 3): (0.22, (-0.9, -0.55, 0.7)),                        # four per lane, half a workgroup
    (36, 33, 20): (0.05, (-0.9, -0.825, 0.5)),                    # the design's: four per lane, 23760 voxels, 12 tiles
    (64, 20, 12): (0.03, (-0.96, -0.3, 0.85)),
    (1024, 1, 1): (1.8 / 1024, (-0.9, -0.9 / 1024, 1.03 - 0.9 / 1024)),
    (1, 1024, 1): (0.8 / 1024, (-0.4 / 1024, -0.4, 1.03 - 0.4 / 1024)),
    (1, 1, 1024): (1.0 / 1024, (-0.5 / 1024, -0.5 / 1024, 0.5)),
    (37, 21, 5): (0.05, (-0.9, -0.5, 0.9)),                       # nx % 4 == 1: one voxel per lane
}
SOURCES = [(24, 16, 1), (70, 33, 3), (64, 20, 2)]


def volume(dims, max_weight=64, trunc=0.2, shift=(0.0, 0.0, 0.0)):
    voxel, origin = VOLUMES[dims]
    return VR.spec(*dims, voxel, tuple(o + d for o, d in zip(origin, shift)), trunc, max_weight)


def side_maps(s, rng):
    shape = (s.frames, s.height, s.width)
    return (rng.random(shape) < 0.85).astype(np.uint8), rng.integers(0, 60, shape).astype(np.uint16)


class Device:
    """the torch buffers of one volume and its surface list: the volume between two margins of 0xA5 (one word further with skew),
    the list pre-filled with 0xA5 (one record further with skew), the count between 0xA5 words"""
    def __init__(self, v, start=None, skew=False):
        import torch
        self.torch, self.v = torch, v
        self.n = v.nx * v.ny * v.nz
        self.off = MARGIN + (4 if skew else 0)
        self.hold = torch.full((4 * self.n + 2 * MARGIN + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.hold.data_ptr() % 16 == 0
        words = np.zeros(self.n, np.uint32) if start is None else np.asarray(start, np.uint32).reshape(-1)
        self.hold[self.off:self.off + 4 * self.n].copy_(torch.from_numpy(words.view(np.uint8)))
        self.skew = skew
        self.points = self.count = None
        torch.cuda.synchronize()

    @property
    def voxels(self):
        return self.hold.data_ptr() + self.off

    def words(self, label):
        raw = self.hold.cpu().numpy()
        lo, hi = self.off, self.off + 4 * self.n
        assert np.all(raw[:lo] == 0xA5) and np.all(raw[hi:] == 0xA5), f"{label}: wrote outside the volume"
        return raw[lo:hi].view(np.uint32).reshape(self.v.nz, self.v.ny, self.v.nx)

    def extract(self, inst, min_weight, capacity, label):
        """(count, the records written): everything behind them, and around the count, still 0xA5"""
        torch = self.torch
        room = capacity + 3
        self.points = torch.full((16 * (room + 1),), 0xA5, dtype=torch.uint8, device="cuda")
        self.count = torch.full((12,), 0xA5, dtype=torch.uint8, device="cuda")
        p_off = 16 if self.skew else 0
        torch.cuda.synchronize()
        assert inst.volume_points(c_volume(self.v), self.voxels, min_weight, self.points.data_ptr() + p_off if capacity else None, capacity,
                                  self.count.data_ptr() + 4), label
        assert inst.synchronize(), label
        c = self.count.cpu().numpy()
        assert np.all(c[:4] == 0xA5) and np.all(c[8:] == 0xA5), f"{label}: wrote around the count"
        count = int(c[4:8].view(np.uint32)[0])
        raw = self.points.cpu().numpy()
        written = min(count, capacity)
        assert np.all(raw[:p_off] == 0xA5) and np.all(raw[p_off + 16 * written:] == 0xA5), f"{label}: wrote outside the {written} records"
        return count, raw[p_off:p_off + 16 * written].view(VR.SURFACE)


def upload(arr, skew=False):
    """a map on the device, optionally one element off a 16-byte boundary"""
    import torch
    if arr is None:
        return None
    flat = np.ascontiguousarray(arr).reshape(-1)
    e = flat.dtype.itemsize
    hold = torch.empty(flat.size * e + 16 + e, dtype=torch.uint8, device="cuda")
    assert hold.data_ptr() % 16 == 0
    view = hold[e if skew else 0:(e if skew else 0) + flat.size * e]
    view.copy_(torch.from_numpy(flat.view(np.uint8)))
    return view


def integrate(inst, dev, s, poses, disp, mask=None, conf=None, skew_maps=False, label=""):
    maps = [upload(m, skew_maps) for m in (disp, mask, conf)]
    dev.torch.cuda.synchronize()
    assert inst.volume_integrate(c_volume(dev.v), c_source(s), poses, *(None if m is None else m.data_ptr() for m in maps), dev.voxels), label
    assert inst.synchronize(), label
    for m, host in zip(maps, (disp, mask, conf)):                 # the inputs are only read
        assert m is None or m.cpu().numpy().tobytes() == np.ascontiguousarray(host).tobytes(), label
    return dev.words(label)


def same_volume(label, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k, j, i = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {got.size} voxels differ, first at (i, j, k) = ({i}, {j}, {k}): "
                             f"{got[k, j, i]:#010x} != {want[k, j, i]:#010x}")


def same_list(label, got, want):
    count, recs = got
    assert count == len(want), f"{label}: {count} crossings, the restatement has {len(want)}"
    assert recs.tobytes() == want[:len(recs)].tobytes(), f"{label}: the surface list differs"


def check(inst, v, s, poses, disp, mask=None, conf=None, start=None, label="", skew=False, skew_maps=False, min_weights=(1,)):
    """one integration and its surface lists against the restatement; returns the volume"""
    dev = Device(v, start, skew)
    got = integrate(inst, dev, s, poses, disp, mask, conf, skew_maps, label)
    want, updates = VR.integrate(VR.empty(v) if start is None else start, v, s, poses, disp, mask, conf)
    same_volume(label, got, want)
    for mw in min_weights:
        pts = VR.crossings(want, v, mw)
        same_list(f"{label} min_weight {mw}", dev.extract(inst, mw, len(pts) + 2, label), pts)
    return want, updates


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: explicit maps need no shape
    yield i
    i.close()


@pytest.mark.parametrize("dims", sorted(VOLUMES))
def test_every_volume_under_every_source_with_and_without_side_maps(inst, dims):
    v = volume(dims)
    for k, (w, h, frames) in enumerate(SOURCES):
        s = camera(w, h, frames=frames, min_conf=9)
        rng = np.random.default_rng(100 * k + dims[0])
        disp = noisy_maps(s, rng)
        mask, conf = side_maps(s, rng)
        for sides in (False, True):
            label = f"{dims} under {w}x{h}x{frames} maps={sides}"
            want, updates = check(inst, v, s, moving_rig(frames), disp, mask if sides else None, conf if sides else None, label=label,
                                  min_weights=(1, 2))
            if not sides:                                         # the case is about something (one masked pixel can hide a whole column)
                assert updates > 0.1 * frames * v.nx * v.ny * v.nz, (label, updates)
                assert max(dims) <= 8 or len(VR.crossings(want, v, 1)) > 0, label


def test_the_designs_scenes(inst):
    v, s, poses, disp = plane_scene()
    want, updates = check(inst, v, s, poses, disp, label="plane")
    assert updates == 20154
    pts = VR.crossings(want, v, 1)
    err = float(np.abs(pts["z"].astype(np.float64) - 1.03).max()) / v.voxel
    print("plane on the device: 612 crossings, max |z - 1.03| = %.3g voxel" % err)
    assert len(pts) == 612 and set(pts["id"] & 3) == {2} and err <= 5e-4
    v, s, poses, disp = noisy_scene()
    want, _ = check(inst, v, s, poses, disp, label="noisy", min_weights=(1, 2))
    assert VR.unpack(want)[1].max() == 2


def test_poses(inst):
    """identity; the rotated pair; a camera looking away, which leaves the volume byte-identical; a volume half outside the frustum"""
    s = camera(70, 33, frames=3, min_conf=9)
    rng = np.random.default_rng(7)
    disp = noisy_maps(s, rng)
    mask, conf = side_maps(s, rng)
    v = volume((36, 33, 20))
    start, _ = check(inst, v, s, np.stack([VR.pose()] * 3), disp, mask, conf, label="identity")
    check(inst, v, s, moving_rig(3), disp, mask, conf, start=start, label="rotated, on a volume with history")
    away = np.stack([VR.pose(rot(1, np.pi)), VR.pose(rot(0, np.pi), (0.0, 0.0, -0.2)), VR.pose(np.eye(3), (0.0, 0.0, -5.0))])
    for skew in (False, True):
        poisoned = np.full((v.nz, v.ny, v.nx), 0x00037FFF, np.uint32)
        dev = Device(v, poisoned, skew)
        got = integrate(inst, dev, s, away, disp, label="looking away")
        assert got.tobytes() == poisoned.tobytes()
        assert VR.integrate(poisoned, v, s, away, disp)[1] == 0
    half = volume((36, 33, 20), shift=(0.9, 0.0, 0.0))
    want, updates = check(inst, half, s, moving_rig(3), disp, label="half outside")
    w = VR.unpack(want)[1]
    assert np.all(w[:, :, -6:] == 0) and w[:, :, :12].max() == 3 and updates > 5000       # the far columns are never seen


def test_pointers_one_element_off(inst):
    """the volume one word off a 16-byte boundary takes one voxel per lane with nx % 4 == 0 too; maps one element off; the list one
    record off"""
    for dims, (w, h, frames) in (((36, 33, 20), (70, 33, 3)), ((64, 20, 12), (64, 20, 2)), ((1024, 1, 1), (24, 16, 1))):
        s = camera(w, h, frames=frames, min_conf=9)
        rng = np.random.default_rng(13 + w)
        disp = noisy_maps(s, rng)
        mask, conf = side_maps(s, rng)
        v = volume(dims, max_weight=2)
        for skew, skew_maps in ((True, False), (False, True), (True, True)):
            check(inst, v, s, moving_rig(frames), disp, mask, conf, label=f"{dims} skew={skew} maps off={skew_maps}", skew=skew, skew_maps=skew_maps)


def test_map_sprinkled_with_nan_and_infinities(inst):
    s = camera(70, 33, frames=3, min_conf=9)
    rng = np.random.default_rng(23)
    disp = noisy_maps(s, rng)
    mask, conf = side_maps(s, rng)
    disp.reshape(-1)[::7] = np.nan
    disp.reshape(-1)[3::11] = -np.inf
    disp.reshape(-1)[5::13] = np.inf
    disp.reshape(-1)[1::17] = np.float32(-1.0)                    # den < 0
    assert np.isnan(disp).sum() > 100 and np.isinf(disp).sum() > 300
    for dims in ((36, 33, 20), (37, 21, 5)):
        check(inst, volume(dims), s, moving_rig(3), disp, label=f"sprinkled {dims}")
        check(inst, volume(dims), s, moving_rig(3), disp, mask, conf, label=f"sprinkled {dims} with side maps")


@pytest.mark.parametrize("max_weight", [1, 3])
def test_integrated_past_saturation(inst, max_weight):
    s = camera(64, 20, frames=2)
    v = volume((64, 20, 12), max_weight=max_weight)
    vox = None
    for k in range(3):                                            # 6 frames on a cap of 1 or 3
        disp = noisy_maps(s, np.random.default_rng(50 + k))
        vox, _ = check(inst, v, s, moving_rig(2), disp, start=vox, label=f"max_weight {max_weight} round {k}", min_weights=(1, max_weight))
    w = VR.unpack(vox)[1]
    assert w.max() == max_weight and (w == max_weight).sum() > 0.3 * w.size


def test_planted_cases(inst):
    v, s, poses, disp, start = planted_scene([p[0] for p in PLANTED])
    want, _ = check(inst, v, s, poses, disp, start=start, label="planted halves")
    assert VR.unpack(want)[0].reshape(-1).tolist() == [p[1] for p in PLANTED]
    v, vox = planted_crossings()
    for mw in (1, 2, 3):
        pts = VR.crossings(vox, v, mw)
        same_list(f"planted crossings, min_weight {mw}", Device(v, vox).extract(inst, mw, len(pts) + 1, "planted crossings"), pts)


def test_batch_equals_frame_by_frame_and_runs_repeat(inst):
    v, s, poses, disp = noisy_scene()
    runs = []
    for _ in range(2):
        dev = Device(v)
        runs.append(integrate(inst, dev, s, poses, disp, label="batch").tobytes())
    assert runs[0] == runs[1]
    dev = Device(v)
    for f in range(s.frames):
        s1 = CR.spec(s.width, s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, frames=1)
        one = integrate(inst, dev, s1, poses[f:f + 1], disp[f:f + 1], label=f"frame {f}")
    assert one.tobytes() == runs[0]
    lists = [dev.extract(inst, 1, 4000, "repeat") for _ in range(2)]
    assert lists[0][0] == lists[1][0] > 1000 and lists[0][1].tobytes() == lists[1][1].tobytes()


@pytest.mark.parametrize("min_weight", [1, 2])
def test_capacity_clips_the_list_and_never_the_count(inst, min_weight):
    v, s, poses, disp = noisy_scene()
    dev = Device(v, skew=True)
    vox = integrate(inst, dev, s, poses, disp, label="noisy")
    pts = VR.crossings(vox, v, min_weight)
    assert len(pts) > 500
    for cap in (0, len(pts), len(pts) - 1):                       # (extract checks that the record after the last stays 0xA5)
        same_list(f"capacity {cap}", dev.extract(inst, min_weight, cap, f"capacity {cap}"), pts)


def test_one_instance_through_a_large_volume_a_small_one_and_a_larger_batch():
    """the tile scratch is reused: nothing of an earlier, larger extraction may show through a later one"""
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)
    try:
        for k, (dims, (w, h, frames)) in enumerate((((64, 20, 12), (64, 20, 2)), ((8, 5, 3), (24, 16, 1)), ((36, 33, 20), (70, 33, 3)),
                                                    ((1, 1, 1024), (24, 16, 1)), ((36, 33, 20), (24, 16, 7)))):
            s = camera(w, h, frames=frames)
            check(i, volume(dims, max_weight=5), s, moving_rig(frames), noisy_maps(s, np.random.default_rng(41 + k)),
                  label=f"step {k}: {dims} under {w}x{h}x{frames}", min_weights=(1, 2))
    finally:
        i.close()


def test_last_match_map_behind_a_match_on_the_device():
    """d_disp == NULL behind match_device, with and without the post pass on a stream of its own: the instance's last final map, the
    one stage 8 reads back -- which match_device does not write (its result goes to the caller's buffer), so a host-pointer match
    fills it first.  And the documented way after match_device: the caller's buffer, read behind the match that is still writing it."""
    import torch
    import soc_project_stereo_matching_amd as S
    z = load_npz("tiny_t70x33_d16.npz")
    left, right = z["left"], z["right"]
    h, w = left.shape
    s = CR.spec(w, h, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=0.25)         # fb = 10: disparities 0.6..10 are depths 1..16
    v = VR.spec(36, 33, 20, 0.1, (-1.8, -1.65, 0.5), 0.4)
    i = S.SGMInstance(0)
    try:
        d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        d_shift = torch.from_numpy(np.roll(left, 3, axis=1)).cuda()              # another pair: another map in the caller's buffer
        d_out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        for overlap in (False, True):
            assert i.set_overlap_post(overlap) and i.reset(w, h, S.default_option(16, min_speckle_area=9))
            assert i.match(left, right) is not None
            own, mine = Device(v), Device(v)
            assert i.match_device(d_shift.data_ptr(), d_r.data_ptr(), d_out.data_ptr())
            assert i.volume_integrate(c_volume(v), c_source(s), VR.pose(), None, None, None, own.voxels)
            assert i.volume_integrate(c_volume(v), c_source(s), VR.pose(), d_out.data_ptr(), None, None, mine.voxels)
            assert i.synchronize()
            final, result = i.read_stage("final"), d_out.cpu().numpy()
            assert np.isfinite(final).sum() > 0.3 * w * h and final.tobytes() != result.tobytes()
            for label, dev, disp in (("the instance's map", own, final), ("the caller's buffer", mine, result)):
                want, updates = VR.integrate(VR.empty(v), v, s, VR.pose()[None], disp.reshape(1, h, w))
                assert updates > 500, (label, updates)
                same_volume(f"{label}, overlap={overlap}", dev.words(label), want)
        other = CR.spec(w, h - 1, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=0.25)
        assert not i.volume_integrate(c_volume(v), c_source(other), VR.pose(), None, None, None, own.voxels)
    finally:
        i.close()


def test_every_refusal_queues_nothing(inst):
    import torch
    v, s, poses, disp = noisy_scene()
    dev = Device(v, np.full(v.nx * v.ny * v.nz, 0xA5A5A5A5, np.uint32))
    d = upload(disp)
    points = torch.full((16 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    count = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    cv, cs = c_volume(v), c_source(s)
    x, q, k = dev.voxels, points.data_ptr(), count.data_ptr()
    nan = float("nan")

    def vol(**kw):
        t = c_volume(v)
        for name, val in kw.items():
            if isinstance(val, tuple):
                getattr(t, name)[val[0]] = val[1]
            else:
                setattr(t, name, val)
        return t

    for n, t in enumerate((vol(nx=0), vol(ny=1025), vol(nz=-1), vol(voxel=0.0), vol(voxel=nan), vol(origin=(1, nan)), vol(trunc=float("inf")),
                           vol(max_weight=0), vol(max_weight=65536))):
        assert not inst.volume_integrate(t, cs, poses, d.data_ptr(), None, None, x), n
        assert not inst.volume_points(t, x, 1, q, 64, k), n
    bad_pose = poses.copy()
    bad_pose[2, 10] = nan
    src65 = CR.spec(s.width, s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, frames=65)
    assert not inst.volume_integrate(cv, cs, bad_pose, d.data_ptr(), None, None, x)
    assert not inst.volume_integrate(cv, c_source(src65), moving_rig(65), d.data_ptr(), None, None, x)
    assert not inst.volume_integrate(cv, cs, poses, d.data_ptr() + 2, None, None, x) and not inst.volume_integrate(cv, cs, poses, d.data_ptr(), None, None, x + 2)
    assert not inst.volume_integrate(cv, cs, poses, d.data_ptr(), None, None, d.data_ptr()) and not inst.volume_integrate(cv, cs, poses, d.data_ptr(), x, None, x)
    assert not inst.volume_integrate(cv, cs, poses, None, None, None, x)                      # no match to take a map from
    assert not inst.volume_points(cv, x, 0, q, 64, k) and not inst.volume_points(cv, x, 65536, q, 64, k)
    assert not inst.volume_points(cv, x, 1, q + 8, 63, k) and not inst.volume_points(cv, x, 1, None, 64, k) and not inst.volume_points(cv, x, 1, q, 64, k + 2)
    assert not inst.volume_points(cv, x, 1, q, 64, x + 16) and not inst.volume_points(cv, x, 1, q, 64, q + 32)
    assert inst.synchronize()
    torch.cuda.synchronize()
    assert bool((dev.hold == 0xA5).all()) and bool((points == 0xA5).all()) and bool((count == 0xA5).all())
    assert d.cpu().numpy().tobytes() == disp.tobytes()


def test_under_guard_bands(monkeypatch):
    """the debug allocation mode around the tile scratch: one tile, then a larger volume on the same instance"""
    import torch
    import soc_project_stereo_matching_amd as S
    assert S.debug_guard_check() == (0, 0, 0)
    monkeypatch.setenv("SGM_DEBUG_GUARD", str(1 << 20))
    monkeypatch.setenv("SGM_DEBUG_POISON", str(0x5A))
    i = S.SGMInstance(0)
    try:
        for k, (dims, (w, h, frames)) in enumerate((((8, 5, 3), (24, 16, 1)), ((36, 33, 20), (70, 33, 3)))):
            s = camera(w, h, frames=frames)
            check(i, volume(dims), s, moving_rig(frames), noisy_maps(s, np.random.default_rng(43 + k)), label=f"guarded {dims}", min_weights=(1, 2))
        torch.cuda.synchronize()
        bad, live, size = S.debug_guard_check()
        assert bad == 0 and live > 0 and size > 0
    finally:
        i.close()
    assert S.debug_guard_check() == (0, 0, 0)
