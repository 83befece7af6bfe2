"""Frame-to-model tracking on the device (extension; include/sgm_mi355x.h, sgm_track_spec; csrc/sgm_track.hip) against the numpy
restatement tests/track_ref.py -- needs an MI355X.  Tolerance 0 everywhere: the sums are exact integers and the poses of sgm_track
are compared bit by bit.  The sums sit between margins of 0xA5, which are checked afterwards, and every input is verified as only
read."""
import numpy as np
import pytest

import cloud_ref as CR
import raycast_ref as RR
import track_ref as TR
import volume_ref as VR
from test_gpu_raycast import Between
from test_gpu_volume import c_source, c_volume
from test_raycast_cpu import c_view
from test_track_cpu import (CORNER_VIEW, IDENTITY, PLANTED_PIXELS, c_model, corner_scene, fused_volume, noisy_case, pose_errors)

pytestmark = pytest.mark.gpu

# source sizes: 65 and 129 leave a partial wave, 257 x 65 takes 66 workgroups a frame; 24 x 16 and 64 x 36 (three workgroups) can be
# read four pixels at a time
SOURCES = [(70, 33), (24, 16), (1, 1), (65, 3), (3, 65), (129, 2), (257, 65), (64, 36)]


class Inputs:
    """the maps of one call on the device, each between margins; skew: the source maps one 4-byte element off a 16-byte boundary"""
    def __init__(self, disp, depth, normal, mask=None, conf=None, skew=False):
        self.host = dict(disp=np.ascontiguousarray(disp, np.float32), depth=np.ascontiguousarray(depth, np.float32),
                         normal=np.ascontiguousarray(normal, np.float32))
        if mask is not None:
            self.host["mask"] = np.ascontiguousarray(mask, np.uint8)
        if conf is not None:
            self.host["conf"] = np.ascontiguousarray(conf, np.uint16)
        self.dev = {k: Between(a.nbytes, a, skew and k in ("disp", "mask", "conf")) for k, a in self.host.items()}

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def only_read(self, label):
        for k, a in self.host.items():
            assert self.dev[k].read(f"{label} {k}").tobytes() == a.tobytes(), f"{label}: {k} is only read"


def device_sums(inst, s, m, poses, inp, label, sums=None):
    """one sgm_track_sums on the device: int64 [frames][29]; the margins and the inputs untouched"""
    import torch
    out = sums or Between(232 * s.frames)
    torch.cuda.synchronize()
    assert inst.track_sums(c_source(s), c_model(m), poses, inp.ptr("disp"), inp.ptr("mask"), inp.ptr("conf"), inp.ptr("depth"),
                           inp.ptr("normal"), out.ptr), label
    assert inst.synchronize(), label
    got = out.read(label + " sums", np.int64).reshape(s.frames, 29).copy()
    inp.only_read(label)
    return got


def check(inst, s, m, poses, disp, depth, normal, mask=None, conf=None, label="", skew=False):
    got = device_sums(inst, s, m, poses, Inputs(disp, depth, normal, mask, conf, skew), label)
    want = TR.sums(disp, s, m, poses, depth, normal, mask, conf)
    assert got.tolist() == want.tolist(), label
    return want


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: tracking needs no shape
    yield i
    i.close()


@pytest.mark.parametrize("size", SOURCES)
def test_sums_for_every_source_and_model(inst, size):
    w, h = size
    total = 0
    for frames, model_size in ((1, (w, h)), (3, (20, 13)), (3, (70, 33))):
        s, disp, m, poses, depth, normal, mask, conf = noisy_case(seed=100 + w, frames=frames, w=w, h=h, model_size=model_size)
        total += int(check(inst, s, m, poses, disp, depth, normal, mask, conf, f"{w}x{h}x{frames} against {model_size}")[:, 28].sum())
        total += int(check(inst, s, m, poses, disp, depth, normal, None, None, f"{w}x{h}x{frames} against {model_size}, no side maps")[:, 28].sum())
    assert total > 100 or w * h < 300, (size, total)              # the cases are about something, except the slivers


def test_64_frames(inst):
    s, disp, m, poses, depth, normal, mask, conf = noisy_case(seed=7, frames=64)
    poses = poses[np.arange(64) % 4]
    want = check(inst, s, m, poses, disp, depth, normal, mask, conf, "64 frames")
    assert (want[:, 28] > 0).sum() > 48


@pytest.mark.parametrize("size", [(24, 16), (64, 36), (70, 33)])
def test_skewed_and_aligned_maps_with_and_without_side_maps(inst, size):
    w, h = size
    s, disp, m, poses, depth, normal, mask, conf = noisy_case(seed=3, frames=3, w=w, h=h)
    seen = {}
    for sides in ("both", "mask", "conf", "none"):
        mk = mask if sides in ("both", "mask") else None
        cf = conf if sides in ("both", "conf") else None
        for skew in (False, True):
            seen[sides, skew] = check(inst, s, m, poses, disp, depth, normal, mk, cf, f"{size} {sides} skew={skew}", skew=skew).tolist()
        assert seen[sides, False] == seen[sides, True]
    assert seen["both", False] != seen["none", False]


@pytest.mark.parametrize("name", sorted(PLANTED_PIXELS))
def test_planted_pixels(inst, name):
    s, disp, m, poses, depth, normal = PLANTED_PIXELS[name]()
    want = check(inst, s, m, poses, disp, depth, normal, label=name)
    assert want[0, 28] == (15 if name == "nothing planted" else 14)


def test_runs_repeat_and_a_batch_equals_frame_by_frame(inst):
    s, disp, m, poses, depth, normal, mask, conf = noisy_case(seed=5, frames=3, w=70, h=33)
    inp = Inputs(disp, depth, normal, mask, conf)
    runs = [device_sums(inst, s, m, poses, inp, "batch") for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
    one = CR.spec(70, 33, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, doffs=s.doffs, z_min=s.z_min, z_max=s.z_max, min_conf=s.min_conf)
    for f in range(3):
        got = device_sums(inst, one, m, poses[f:f + 1], Inputs(disp[f], depth[f], normal[f], mask[f], conf[f]), f"frame {f}")
        assert got[0].tobytes() == runs[0][f].tobytes(), f


def test_no_association_gives_zeros_and_status_1(inst):
    s, disp, m, depth, normal, _ = corner_scene(3, frames=2)
    disp = np.full_like(disp, np.inf)
    inp = Inputs(disp, depth, normal)
    got = device_sums(inst, s, m, np.stack([IDENTITY, IDENTITY]).astype(np.float32), inp, "empty")
    assert not got.any()
    guess = np.stack([IDENTITY, IDENTITY])
    poses, stats = inst.track(c_source(s), c_model(m), guess, inp.ptr("disp"), None, None, inp.ptr("depth"), inp.ptr("normal"))
    assert stats == [dict(pixels=0, rms=0.0, status=1)] * 2 and poses.tobytes() == guess.tobytes()
    # all behind the model camera: the same
    s, disp, m, depth, normal, _ = corner_scene(1)
    away = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -5], np.float32)
    assert not check(inst, s, m, away[None], disp, depth, normal, label="behind").any()


def test_sgm_track_round_by_round_on_the_room_corner(inst):
    """a converging frame, one that associates nothing and one that sees a single plane, in one call of four rounds"""
    s, disp, m, depth, normal, true = corner_scene(4, frames=3)
    disp, depth, normal = disp.copy(), depth.copy(), normal.copy()
    disp[1] = np.inf
    depth[2], normal[2], disp[2] = 2.0, (0.0, 0.0, -1.0), 20.0
    guess = np.stack([IDENTITY, IDENTITY, IDENTITY])
    inp = Inputs(disp, depth, normal)
    got = inst.track(c_source(s), c_model(m), guess, inp.ptr("disp"), None, None, inp.ptr("depth"), inp.ptr("normal"), trace=True)
    assert got is not None
    poses, stats, t_sums, t_poses = got
    inp.only_read("track")
    assert t_poses[0].tobytes() == guess.tobytes() and t_poses[4].tobytes() == poses.tobytes()
    live = [True] * 3
    for i in range(4):
        want = TR.sums(disp, s, m, t_poses[i].astype(np.float32), depth, normal)
        assert t_sums[i].tolist() == want.tolist(), i
        for f in range(3):
            step, st = TR.solve(m, want[f], t_poses[i, f])
            live[f] = live[f] and st["status"] == 0               # a frame whose solve failed sits out and keeps its pose
            assert t_poses[i + 1, f].tobytes() == (np.array(step, np.float64) if live[f] else t_poses[i, f]).tobytes(), (i, f)
    assert [st["status"] for st in stats] == [0, 1, 2]
    w_poses, w_stats, w_sums, w_trace = TR.track(disp, s, m, guess, depth, normal)
    assert poses.tobytes() == w_poses.tobytes() and stats == w_stats and t_poses.tobytes() == w_trace.tobytes() and t_sums.tobytes() == w_sums.tobytes()
    # six rounds of the one frame: the final pose equals the restatement's, which converged (tests/test_track_cpu.py)
    s, disp, m, depth, normal, true = corner_scene(6)
    inp = Inputs(disp, depth, normal)
    poses, stats = inst.track(c_source(s), c_model(m), IDENTITY[None], inp.ptr("disp"), None, None, inp.ptr("depth"), inp.ptr("normal"))
    want, want_stats, _, _ = TR.track(disp, s, m, IDENTITY[None], depth, normal)
    assert poses.tobytes() == want.tobytes() and stats == want_stats
    err = pose_errors(poses[0], true[:9].reshape(3, 3), true[9:])
    assert err[0] < 0.039 / 100 and err[1] < 0.0707 / 100


def test_track_queued_behind_a_raycast_reads_the_finished_maps(inst):
    """ray-cast and sums queued back to back on the instance's stream, no wait in between"""
    import torch
    v, vox, s0 = fused_volume()
    s, disp, m, _, _, _ = corner_scene(1)
    px = CORNER_VIEW.width * CORNER_VIEW.height
    d_vox = Between(vox.nbytes, vox)
    d_depth, d_normal = Between(4 * px), Between(12 * px)
    d_disp, d_sums = Between(disp.nbytes, disp), Between(232)
    torch.cuda.synchronize()
    assert inst.volume_raycast(c_volume(v), c_view(CORNER_VIEW), VR.pose()[None], d_vox.ptr, d_depth.ptr, d_normal.ptr)
    assert inst.track_sums(c_source(s), c_model(m), IDENTITY.astype(np.float32)[None], d_disp.ptr, None, None, d_depth.ptr, d_normal.ptr, d_sums.ptr)
    assert inst.synchronize()
    depth, normal, _ = RR.raycast(vox, v, CORNER_VIEW, VR.pose()[None])
    assert d_depth.read("depth", np.float32).tobytes() == depth.tobytes()
    want = TR.sums(disp, s, m, IDENTITY[None], depth, normal)
    assert want[0, 28] > 1500 and d_sums.read("sums", np.int64).tolist() == want[0].tolist()


def test_every_refusal_queues_nothing(inst):
    import torch
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    inp = Inputs(disp, depth, normal, mask, conf)
    sums = Between(232 * s.frames)
    cs, cm = c_source(s), c_model(m)
    a = [inp.ptr(k) for k in ("disp", "mask", "conf", "depth", "normal")]

    def call(cs=cs, cm=cm, poses=poses, a=a, out=sums.ptr):
        return inst.track_sums(cs, cm, poses, a[0], a[1], a[2], a[3], a[4], out)

    for field, v in (("width", 0), ("height", 65536), ("fx", 0.0), ("cy", float("nan")), ("dist_max", 0.0), ("span", float("inf")),
                     ("iterations", 0), ("min_pixels", 5), ("min_pivot", -1.0)):
        bad = c_model(m)
        setattr(bad, field, v)
        assert not call(cm=bad), field
    large = c_source(s)
    large.width, large.height, large.frames = 4097, 4096, 1
    bad_pose = poses.copy()
    bad_pose[1, 3] = np.nan
    assert not call(cs=large, poses=poses[:1]) and not call(poses=bad_pose)
    assert not call(out=sums.ptr + 4) and not call(out=a[3] & ~7) and not call(out=a[0] & ~7)
    assert not call(a=[a[0] + 2] + a[1:]) and not call(a=a[:3] + [None, a[4]]) and not call(a=[None] + a[1:])
    assert inst.synchronize()
    torch.cuda.synchronize()
    assert bool((sums.hold == 0xA5).all())
    inp.only_read("refusals")
