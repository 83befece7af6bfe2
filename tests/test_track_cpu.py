"""Frame-to-model tracking (extension; include/sgm_mi355x.h, sgm_track_spec) without a GPU: the numpy restatement tests/track_ref.py
against a plain per-pixel loop, a planted pixel for every skip rule, the rounding, the solve, the Cayley step, header / library /
Python agreement, the C host's logic on the stand-in device (tests/stub_device.c + tests/stub_track.c), convergence on an analytic
room corner, the loop integrate -> ray-cast -> track once on the restatements, and a sanitizer run of a stand-alone driver.
Tolerance 0 wherever the stand-in is compared with the restatement."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import raycast_ref as RR
import standin
import track_ref as TR
import volume_ref as VR
from conftest import ROOT
from test_cloud_cpu import f32, div32
from test_volume_cpu import c_source

STUB_TRACK = os.path.join(ROOT, "tests", "stub_track.c")
_p, _i, _b = C.c_void_p, C.c_int, C.c_bool
INF, NAN = float("inf"), float("nan")
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


# ---- scenes --------------------------------------------------------------------------------------------------------------------

def rodrigues(w):
    """the rotation of the rotation vector w, float64"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def pose_of(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def pose_errors(pose, R_true, t_true):
    """(rotation error as an angle, translation error as a length) of a [12] pose"""
    pose = np.asarray(pose, np.float64)
    dR = pose[:9].reshape(3, 3) @ np.asarray(R_true).T
    return math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))), float(np.linalg.norm(pose[9:] - np.asarray(t_true)))


# the room corner: three planes (a normal towards free space, the plane n.p = d)
CORNER = [((0.0, -1.0, 0.0), -0.5), ((0.0, 0.0, -1.0), -2.0), ((-1.0, 0.0, 0.0), -0.8)]        # y = 0.5, z = 2, x = 0.8
CORNER_ROT, CORNER_T = (0.02, -0.03, 0.015), (0.04, -0.03, 0.05)


def corner_seen(w, h, fx, fy, cx, cy, R=np.eye(3), t=(0.0, 0.0, 0.0)):
    """the corner from a camera whose points are P_corner = R P_cam + t: (depth [h][w], normal in camera coordinates [h][w][3]) float32"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1) @ np.asarray(R, np.float64).T      # directions in the corner's frame
    best = np.full((h, w), np.inf)
    normal = np.zeros((h, w, 3))
    for n, dist in CORNER:
        n = np.asarray(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = (dist - n @ np.asarray(t, np.float64)) / (d @ n)
        hit = np.isfinite(z) & (z > 0) & (z < best)
        best[hit] = z[hit]
        normal[hit] = np.asarray(R, np.float64).T @ n
    return best.astype(np.float32), normal.astype(np.float32)


def corner_scene(iterations=6, rot=CORNER_ROT, t=CORNER_T, w=70, h=33, frames=1):
    """(source spec, disp, model, model depth, model normal, true pose source -> model): the issue's scene, the same in every frame"""
    fx = fy = 40.0 * w / 70.0
    cx, cy = (w - 1) / 2.0, 16.0 * h / 33.0
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=1.0, frames=frames)
    m = TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, iterations=iterations)
    depth, normal = corner_seen(70, 33, 40.0, 40.0, 34.5, 16.0)
    R = rodrigues(rot)
    z, _ = corner_seen(w, h, fx, fy, cx, cy, R, t)
    disp = (CR.fb_of(s) / z).astype(np.float32)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (frames,) + a.shape))
    return s, rep(disp), m, rep(depth), rep(normal), pose_of(R, t)


# ---- the restatement against a plain loop --------------------------------------------------------------------------------------

def loop_sums(disp, s, m, poses, depth, normal, mask=None, conf=None):
    """The definition of include/sgm_mi355x.h as a loop over Python floats and ints: sums, products and quotients of two float32
    values are exact or correctly rounded in double, so rounding each to float32 once is the float32 operation."""
    F = lambda v: float(np.float32(v))
    fb = float(CR.fb_of(s))
    sfx, sfy, scx, scy, doffs, z_min, z_max = (F(x) for x in (s.fx, s.fy, s.cx, s.cy, s.doffs, s.z_min, s.z_max))
    fx, fy, cx, cy, dist_max, span = (F(x) for x in (m.fx, m.fy, m.cx, m.cy, m.dist_max, m.span))
    gate = f32(dist_max * dist_max)
    disp = np.asarray(disp, np.float32).reshape(s.frames, s.height, s.width)
    depth = np.asarray(depth, np.float32).reshape(s.frames, m.height, m.width)
    normal = np.asarray(normal, np.float32).reshape(s.frames, m.height, m.width, 3)
    out = []
    for fr in range(s.frames):
        P = [float(x) for x in np.asarray(poses, np.float32).reshape(-1, 12)[fr]]
        acc = [0] * 29
        for y in range(s.height):
            for x in range(s.width):
                d = float(disp[fr, y, x])
                if not math.isfinite(d) or (mask is not None and mask[fr, y, x] == 0) or (conf is not None and int(conf[fr, y, x]) < s.min_conf):
                    continue
                den = f32(d + doffs)
                if not (math.isfinite(den) and den > 0):
                    continue
                Z = div32(fb, den)
                if not (math.isfinite(Z) and z_min <= Z <= z_max):
                    continue
                X, Y = div32(f32(f32(float(x) - scx) * Z), sfx), div32(f32(f32(float(y) - scy) * Z), sfy)
                Px, Py, Pz = (f32(f32(f32(f32(P[3 * r] * X) + f32(P[3 * r + 1] * Y)) + f32(P[3 * r + 2] * Z)) + P[9 + r]) for r in range(3))
                if not math.isfinite(Pz) or not Pz > 0:
                    continue
                u, v = f32(f32(fx * div32(Px, Pz)) + cx), f32(f32(fy * div32(Py, Pz)) + cy)
                if not (math.isfinite(u) and math.isfinite(v)):
                    continue
                uf, vf = math.floor(f32(u + 0.5)), math.floor(f32(v + 0.5))
                if not (0 <= uf < m.width and 0 <= vf < m.height):
                    continue
                Zm = float(depth[fr, vf, uf])
                n = [float(c) for c in normal[fr, vf, uf]]
                if not (math.isfinite(Zm) and Zm > 0 and all(math.isfinite(c) for c in n)):
                    continue
                e = [f32(div32(f32(f32(float(uf) - cx) * Zm), fx) - Px), f32(div32(f32(f32(float(vf) - cy) * Zm), fy) - Py), f32(Zm - Pz)]
                d2 = f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2]))
                if not (math.isfinite(d2) and d2 <= gate):
                    continue
                r = f32(f32(f32(n[0] * e[0]) + f32(n[1] * e[1])) + f32(n[2] * e[2]))
                c = [f32(f32(Py * n[2]) - f32(Pz * n[1])), f32(f32(Pz * n[0]) - f32(Px * n[2])), f32(f32(Px * n[1]) - f32(Py * n[0]))]
                val = [div32(c[0], span), div32(c[1], span), div32(c[2], span), n[0], n[1], n[2], div32(r, dist_max)]
                if not all(math.isfinite(t) and abs(t) <= 8.0 for t in val):
                    continue
                q = [round(t * 65536.0) for t in val]             # the product is exact; Python's round is half to even
                k = 0
                for i in range(7):
                    for j in range(i, 7):
                        acc[k] += q[i] * q[j]
                        k += 1
                acc[28] += 1
        out.append(acc)
    return out


def noisy_case(seed=11, frames=3, w=24, h=16, model_size=(20, 13)):
    """a corner scene seen by a small camera, with noise on the maps, non-finite entries everywhere they may occur and side maps"""
    rng = np.random.default_rng(seed)
    s, disp, m, depth, normal, true = corner_scene(1, w=w, h=h, frames=frames)
    s = CR.spec(w, h, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=1.0, doffs=0.125, frames=frames, z_min=0.3, z_max=1.95, min_conf=9)
    mw, mh = model_size
    m = TR.model(mw, mh, 40.0 * mw / 70.0, 40.0 * mw / 70.0, (mw - 1) / 2.0, 16.0 * mh / 33.0, 0.3, 4.0)
    depth, normal = corner_seen(mw, mh, m.fx, m.fy, m.cx, m.cy)
    depth = np.stack([depth] * frames) + rng.uniform(-0.05, 0.05, (frames, mh, mw)).astype(np.float32)
    normal = np.stack([normal] * frames) + rng.uniform(-0.1, 0.1, (frames, mh, mw, 3)).astype(np.float32)
    disp = (disp + rng.uniform(-0.3, 0.3, disp.shape)).astype(np.float32)
    disp[rng.random(disp.shape) < 0.05] = INF
    disp[0, 1 % h, 2 % w] = NAN
    depth[rng.random(depth.shape) < 0.05] = NAN
    depth[0, 2 % mh, 3 % mw], depth[0, 2 % mh, 4 % mw], depth[-1, 0, 0] = 0.0, -1.0, INF
    normal[rng.random(normal.shape) < 0.02] = NAN
    normal[-1, 1 % mh, 1 % mw, 2] = INF
    mask = (rng.random(disp.shape) < 0.85).astype(np.uint8)
    conf = rng.integers(0, 60, disp.shape).astype(np.uint16)
    poses = np.stack([pose_of(rodrigues(np.array(CORNER_ROT) * k / 2), np.array(CORNER_T) * k / 2) for k in range(frames)]).astype(np.float32)
    return s, disp, m, poses, depth.astype(np.float32), normal.astype(np.float32), mask, conf


@pytest.mark.parametrize("sides", [False, True])
def test_restatement_equals_the_loop(sides):
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    if not sides:
        mask = conf = None
    got = TR.sums(disp, s, m, poses, depth, normal, mask, conf)
    want = loop_sums(disp, s, m, poses, depth, normal, mask, conf)
    assert got.tolist() == want
    assert all(row[28] > 30 for row in want) and all(row[28] < s.width * s.height for row in want)      # the case is about something


# ---- a planted pixel for every skip rule ---------------------------------------------------------------------------------------

PLANT_AT = (1, 3)                                                 # (y, x) of the planted pixel of a 5 x 3 source


def planted(disp=2.0, planted_disp=None, pose=IDENTITY, model_w=5, model_fx=4.0, model_depth=2.0, depth_at=None, normal_at=None,
            dist_max=0.5, span=4.0):
    """a 5 x 3 source with fb = 4 that sees a wall at Z = 4 / disp, and a model wall with normal (0, 0, -1); what is planted goes
    to pixel PLANT_AT of the source and, for the model's maps, to the model pixel it lands on under the identity"""
    s = CR.spec(5, 3, fx=4.0, fy=4.0, cx=2.0, cy=1.0, baseline=1.0)
    m = TR.model(model_w, 3, model_fx, model_fx, 2.0, 1.0, dist_max, span)
    d = np.full((1, 3, 5), disp, np.float32)
    if planted_disp is not None:
        d[(0,) + PLANT_AT] = planted_disp
    depth = np.full((1, 3, model_w), model_depth, np.float32)
    normal = np.zeros((1, 3, model_w, 3), np.float32)
    normal[..., 2] = -1.0
    if depth_at is not None:
        depth[(0,) + PLANT_AT] = depth_at
    if normal_at is not None:
        normal[(0,) + PLANT_AT + (normal_at[0],)] = normal_at[1]
    return s, d, m, np.asarray(pose, np.float32)[None], depth, normal


# name: the scene, in which every pixel but the planted one is associated
PLANTED_PIXELS = {
    "nothing planted": lambda: planted(),
    "not KEPT": lambda: planted(planted_disp=INF),
    # t_z = -2.05: the planted Z = 2 ends at Pz = -0.05, the others (Z = 2.5) at 0.45, where a model of fx = 4 * 0.45 / 2.5 sees them
    "behind the camera": lambda: planted(disp=1.6, planted_disp=2.0, pose=pose_of(np.eye(3), (0, 0, -2.05)), model_fx=0.72, model_depth=0.45),
    # t_x = 0.6 moves a pixel at Z by 2.4 / Z columns: one at Z = 2, five at Z = 0.5, which leaves a model of 6 columns
    "outside the model": lambda: planted(planted_disp=8.0, pose=pose_of(np.eye(3), (0.6, 0, 0)), model_w=6),
    "NaN model depth": lambda: planted(depth_at=NAN),
    "NaN normal component": lambda: planted(normal_at=(1, NAN)),
    # e = (-0.15, 0, -0.6): 0.3825 > 0.25
    "beyond the gate": lambda: planted(planted_disp=4.0 / 2.6),
    # span 0.15: Px = 1 in the last column is c1 / span = 6.67 (|q| > 2^18), the planted Z = 5 has Px = 1.25: 8.33
    "|v_i| > 8": lambda: planted(planted_disp=0.8, dist_max=4.0, span=0.15),
}


@pytest.mark.parametrize("name", sorted(PLANTED_PIXELS))
def test_planted_pixel(name):
    s, disp, m, poses, depth, normal = PLANTED_PIXELS[name]()
    ok, q = TR.quantised(disp[0], s, m, poses[0], depth[0], normal[0])
    want = np.ones((3, 5), bool)
    if name != "nothing planted":
        want[PLANT_AT] = False
    assert np.array_equal(ok, want), (name, ok)
    assert TR.sums(disp, s, m, poses, depth, normal).tolist() == loop_sums(disp, s, m, poses, depth, normal)
    if name == "|v_i| > 8":
        assert np.abs(q).max() > 1 << 18 and np.abs(q).max() <= 1 << 19


def test_rint_rounds_half_to_even():
    """normals of 1.5 / 65536 and 2.5 / 65536: both products are exact halves and both round to 2"""
    s, disp, m, poses, depth, normal = planted()
    normal[0, 1, 3, 0], normal[0, 1, 3, 1] = 1.5 / 65536, 2.5 / 65536
    normal[0, 1, 2, 0], normal[0, 1, 2, 1] = -0.5 / 65536, -3.5 / 65536
    ok, q = TR.quantised(disp[0], s, m, poses[0], depth[0], normal[0])
    assert ok.all() and q[1, 3, 3:6].tolist() == [2, 2, -65536] and q[1, 2, 3:6].tolist() == [0, -4, -65536]
    assert TR.sums(disp, s, m, poses, depth, normal).tolist() == loop_sums(disp, s, m, poses, depth, normal)


# ---- the solve -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corner_sums():
    s, disp, m, depth, normal, _ = corner_scene()
    got = TR.sums(disp, s, m, IDENTITY[None], depth, normal)[0]
    got.setflags(write=False)
    return m, got


def matrix_of(sums29):
    A = np.zeros((7, 7))
    for k, (i, j) in enumerate(TR.PAIRS):
        A[i, j] = A[j, i] = float(int(sums29[k]))
    return A


def test_solve_against_numpy():
    m, sums29 = corner_sums()
    assert sums29[28] > 2000
    pose, stats = TR.solve(m, sums29, IDENTITY)
    assert stats["status"] == 0 and stats["pixels"] == sums29[28]
    A = matrix_of(sums29)
    xi = np.linalg.solve(A[:6, :6], A[:6, 6])
    dist_max = float(np.float32(0.3))                            # the spec's fields are float32
    w, v = xi[:3] * (dist_max / 4.0), xi[3:] * dist_max
    # the Cayley map of w / 2 against its closed form (I - S)^-1 (I + S), S = [w / 2]x
    S = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / 2
    want_R = np.linalg.inv(np.eye(3) - S) @ (np.eye(3) + S)
    assert np.allclose(np.array(pose[:9]).reshape(3, 3), want_R, rtol=0, atol=1e-9) and np.allclose(pose[9:], v, rtol=1e-6, atol=1e-12)
    assert stats["rms"] == pytest.approx(dist_max * math.sqrt(int(sums29[27]) / int(sums29[28])) / 65536, rel=1e-15)
    # a second pose in: R' = Ri R, t' = Ri t + v
    start = pose_of(rodrigues((0.3, -0.2, 0.5)), (1.0, -2.0, 0.5))
    pose2, _ = TR.solve(m, sums29, start)
    assert np.allclose(np.array(pose2[:9]).reshape(3, 3), want_R @ start[:9].reshape(3, 3), rtol=0, atol=1e-9)
    assert np.allclose(pose2[9:], want_R @ start[9:] + v, rtol=0, atol=1e-9)


def test_the_cayley_step_is_orthonormal():
    m, sums29 = corner_sums()
    pose = IDENTITY
    big = TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 30.0, 0.5)    # the same xi as a rotation 800 times larger
    for mm in (m, big):
        pose, stats = TR.solve(mm, sums29, pose)
        R = np.array(pose[:9]).reshape(3, 3)
        assert stats["status"] == 0 and np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14) and np.linalg.det(R) == pytest.approx(1.0, abs=1e-14)
    assert pose_errors(pose, np.eye(3), (0, 0, 0))[0] > 1.0


def test_too_few_pixels_and_a_single_plane():
    m, sums29 = corner_sums()
    few = TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, min_pixels=int(sums29[28]) + 1)
    pose, stats = TR.solve(few, sums29, IDENTITY)
    assert stats["status"] == 1 and stats["pixels"] == sums29[28] and stats["rms"] > 0 and list(pose) == IDENTITY.tolist()
    assert TR.solve(TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, min_pixels=int(sums29[28])), sums29, IDENTITY)[1]["status"] == 0
    # one plane seen head on leaves three of the six unknowns open: columns of zeros
    s, disp, mp, poses, depth, normal = planted()
    plane = TR.sums(disp, s, mp, poses, depth, normal)[0]
    assert plane[28] == 15
    pose, stats = TR.solve(mp, plane, IDENTITY)
    assert stats["status"] == 2 and list(pose) == IDENTITY.tolist()
    # ... and a pivot threshold decides the nearly degenerate: the corner passes 1e-6 and fails 0.5
    assert TR.solve(TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, min_pivot=1e-6), sums29, IDENTITY)[1]["status"] == 0
    assert TR.solve(TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, min_pivot=0.5), sums29, IDENTITY)[1]["status"] == 2
    assert TR.solve(m, [0] * 29, IDENTITY)[1] == dict(pixels=0, rms=0.0, status=1)


# ---- convergence ---------------------------------------------------------------------------------------------------------------

def test_the_restatement_converges_on_the_room_corner():
    """The issue's scene: both errors shrink strictly in each of the first three iterations and end below 1 / 100 of their start
    after six.  (A float64 prototype reached 1 / 980 and 1 / 2200.)"""
    s, disp, m, depth, normal, true = corner_scene(6)
    R_true, t_true = true[:9].reshape(3, 3), true[9:]
    _, stats, _, trace = TR.track(disp, s, m, IDENTITY[None], depth, normal)
    errors = [pose_errors(p[0], R_true, t_true) for p in trace]
    print("room corner: (rotation, translation) error per iteration", errors, "pixels", stats[0]["pixels"])
    assert stats[0]["status"] == 0 and stats[0]["pixels"] > 2000
    for k in range(3):
        assert errors[k + 1][0] < errors[k][0] and errors[k + 1][1] < errors[k][1], (k, errors)
    assert errors[6][0] < errors[0][0] / 100 and errors[6][1] < errors[0][1] / 100, errors


CORNER_VIEW = RR.view(70, 33, 40.0, 40.0, 34.5, 16.0, 0.4, 2.3, 0.05)


@functools.lru_cache(maxsize=None)
def fused_volume():
    """frame 0 of a rig in the room corner integrated into a volume by the restatement: (volume spec, words, source spec)"""
    v = VR.spec(56, 36, 36, 0.05, (-1.9, -1.0, 0.5), 0.4)          # (a trunc of 0.2 leaves the grazing floor without normals)
    s = CR.spec(70, 33, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=1.0)
    z0, _ = corner_seen(70, 33, 40.0, 40.0, 34.5, 16.0)
    vox, updates = VR.integrate(VR.empty(v), v, s, VR.pose()[None], (CR.fb_of(s) / z0).astype(np.float32)[None])
    assert updates > 10000
    vox.setflags(write=False)
    return v, vox, s


@functools.lru_cache(maxsize=None)
def fused_corner():
    """... and ray-cast from pose 0: (source spec, depth, normal)"""
    v, vox, s = fused_volume()
    depth, normal, stats = RR.raycast(vox, v, CORNER_VIEW, VR.pose()[None])
    assert stats["normals"] > 1500
    return s, depth, normal


def test_the_loop_once_on_the_restatements():
    """integrate frame 0, ray-cast at pose 0, track frame 1 from pose 0, sgm_track_world_pose: nearer the rig's pose than the guess"""
    s, depth, normal = fused_corner()
    R, t = rodrigues(CORNER_ROT), np.array(CORNER_T)              # camera 1 -> camera 0 (the world)
    z1, _ = corner_seen(70, 33, 40.0, 40.0, 34.5, 16.0, R, t)
    m = TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, iterations=6)
    rel, stats, _, _ = TR.track((CR.fb_of(s) / z1).astype(np.float32)[None], s, m, IDENTITY[None], depth, normal)
    assert stats[0]["status"] == 0 and stats[0]["pixels"] > 1000
    world = TR.world_pose(VR.pose(), rel[0])                      # world -> camera 1
    assert world.dtype == np.float32
    R_true, t_true = R.T, -R.T @ t
    got, guess = pose_errors(world, R_true, t_true), pose_errors(VR.pose(), R_true, t_true)
    print("the loop once: (rotation, translation) error of the guess", guess, "of the tracked pose", got, "stats", stats[0])
    assert got[0] < guess[0] and got[1] < guess[1], (got, guess)


def test_world_pose_inverts_and_composes():
    rel = pose_of(rodrigues((0.1, -0.2, 0.05)), (0.3, -0.1, 0.2))
    model_pose = pose_of(rodrigues((-0.3, 0.1, 0.2)), (1.0, 2.0, -0.5)).astype(np.float32)
    got = TR.world_pose(model_pose, rel)
    Rr, tr, Rm, tm = rel[:9].reshape(3, 3), rel[9:], model_pose[:9].reshape(3, 3).astype(np.float64), model_pose[9:].astype(np.float64)
    assert np.allclose(got[:9].reshape(3, 3), Rr.T @ Rm, rtol=0, atol=1e-6) and np.allclose(got[9:], Rr.T @ (tm - tr), rtol=0, atol=1e-6)


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


FIELDS = ["width", "height", "fx", "fy", "cx", "cy", "dist_max", "span", "iterations", "min_pixels", "min_pivot"]


def c_model(m):
    import soc_project_stereo_matching_amd as S
    return S.track_spec(m.width, m.height, m.fx, m.fy, m.cx, m.cy, m.dist_max, m.span, m.iterations, m.min_pixels, m.min_pivot)


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    for name in ("sgm_track_sums", "sgm_track_solve", "sgm_track", "sgm_track_world_pose"):
        assert name in _declared_functions() and hasattr(lib, name), name
    assert hasattr(lib, "sgmd_track_sums")
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    block = text.split("frame-to-model tracking: projective point-to-plane ICP against the ray-cast")[1].split("sgm_track_spec;")[0]
    assert text.index("sgm_raycast_spec;") < text.index("frame-to-model tracking: projective point-to-plane ICP") < text.index("sgm_scale_spec;")
    for line in ("Px = ((R0*X + R1*Y) + R2*Z) + t0", "u = fx*(Px/Pz) + cx,  v = fy*(Py/Pz) + cy", "uf = floorf(u + 0.5f), vf = floorf(v + 0.5f)",
                 "Q  = (((uf - cx)*Zm)/fx, ((vf - cy)*Zm)/fy, Zm)", "(e0*e0 + e1*e1) + e2*e2", "r  = (n0*e0 + n1*e1) + n2*e2",
                 "c0 = Py*n2 - Pz*n1,  c1 = Pz*n0 - Px*n2,  c2 = Px*n1 - Py*n0", "v[0..6] = c0/span, c1/span, c2/span, n0, n1, n2, r/dist_max",
                 "|v_i| <= 8.0f", "q_i = (int32)rintf(v_i * 65536.0f)", "J = [P x n, n]", "2^24", "2^62",
                 "D_j  = A_jj - sum_{k<j} (L_jk*L_jk)*D_k", "D_j > min_pivot * A_jj", "L_ij = (A_ij - sum_{k<j} (L_ik*L_jk)*D_k) / D_j",
                 "w_i = xi_i * (dist_max / span),   v_i = xi_{3+i} * dist_max", "Ri_rc = ((a*I_rc + 2*(s_r*s_c)) + 2*X_rc) / den",
                 "t'_r = ((Ri_r0*t0 + Ri_r1*t1) + Ri_r2*t2) + v_r", "rms = dist_max * sqrt("):
        assert line in block, line
    for out in ("image pyramids", "robust weights", "normal-angle gate", "photometric", "loop closure", "row tiles", "sgm_match_planes"):
        assert out in block.split("Not part of it:")[1], out
    assert C.sizeof(S.SGMTrackSpec) == 44 and C.sizeof(S.SGMTrackStats) == 16
    assert [f[0] for f in S.SGMTrackSpec._fields_] == FIELDS
    assert [getattr(S.SGMTrackSpec, n).offset for n in FIELDS] == list(range(0, 44, 4))
    assert [(n, getattr(S.SGMTrackStats, n).offset) for n, _ in S.SGMTrackStats._fields_] == [("rms", 0), ("pixels", 8), ("status", 12)]
    body = re.search(r"typedef struct \{([^}]*)\} sgm_track_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == FIELDS
    assert re.search(r"typedef struct \{ double rms; uint32_t pixels; int32_t status; \} sgm_track_stats;", text)
    assert callable(getattr(S.SGMInstance, "track_sums", None)) and callable(getattr(S.SGMInstance, "track", None))
    t = S.track_spec(70, 33, 40.0, 41.0, 34.5, 16.0, 0.25, 4.0, 5, 100, 0.5)
    assert (t.width, t.height, t.fx, t.fy, t.cx, t.cy, t.dist_max, t.span, t.iterations, t.min_pixels, t.min_pivot) == \
        (70, 33, 40.0, 41.0, 34.5, 16.0, 0.25, 4.0, 5, 100, 0.5)


def test_the_librarys_solve_and_world_pose_equal_the_restatement(lib, capfd):
    import soc_project_stereo_matching_amd as S
    m, sums29 = corner_sums()
    s, disp, mp, poses, depth, normal = planted()
    plane = TR.sums(disp, s, mp, poses, depth, normal)[0]
    start = pose_of(rodrigues((0.3, -0.2, 0.5)), (1.0, -2.0, 0.5))
    for mm, sm, pose in ((m, sums29, IDENTITY), (m, sums29, start), (mp, plane, start), (m, np.zeros(29, np.int64), IDENTITY),
                         (TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.3, 4.0, min_pivot=0.5), sums29, start)):
        got_pose, got_stats = S.track_solve(c_model(mm), sm, pose)
        want_pose, want_stats = TR.solve(mm, sm, pose)
        assert got_pose.tobytes() == np.array(want_pose, np.float64).tobytes() and got_stats == want_stats
    model_pose = pose_of(rodrigues((-0.3, 0.1, 0.2)), (1.0, 2.0, -0.5)).astype(np.float32)
    assert S.track_world_pose(model_pose, start).tobytes() == TR.world_pose(model_pose, start).tobytes()
    capfd.readouterr()
    bad = start.copy()
    bad[4] = NAN
    assert S.track_solve(c_model(m), sums29, bad) is None and S.track_world_pose(model_pose, bad) is None
    assert S.track_solve(c_model(TR.model(70, 33, 40.0, 40.0, 34.5, 16.0, 0.0, 4.0)), sums29, start) is None
    # a pixel count no launch can give: negative, or above the 2^24 the sums are sized for; 2^24 itself is taken
    for count, taken in ((-1, False), ((1 << 24) + 1, False), (1 << 24, True)):
        odd = sums29.copy()
        odd[28] = count
        assert (S.track_solve(c_model(m), odd, start) is not None) == taken, count
    err = capfd.readouterr().err
    assert err.count("sgm_mi355x: sgm_track_solve:") == 4 and err.count("associated pixels (0..2^24)") == 2
    assert err.count("sgm_mi355x: sgm_track_world_pose:") == 1


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

class DeviceCloud(C.Structure):                                  # sgmd_cloud of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i), ("B", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "fb", "doffs", "z_min", "z_max")] + \
               [("min_conf", C.c_uint)]


class DeviceTrack(C.Structure):                                  # sgmd_track of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "dist_max", "span")]


def _sign(L):
    for name, (res, args) in {"sgm_track_sums": (_b, [_p] * 10), "sgm_track": (_b, [_p] * 12), "sgm_track_solve": (_b, [_p] * 5),
                              "stub_track_clear": (None, []), "stub_track_count": (_i, []), "stub_track_ptr": (_p, [_i, _i]),
                              "stub_track_source": (C.POINTER(DeviceCloud), [_i]), "stub_track_model": (C.POINTER(DeviceTrack), [_i]),
                              "stub_track_poses": (C.POINTER(C.c_float), [_i]), "stub_track_fail_at": (None, [_i])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("trackstub"), extra_sources=[STUB_TRACK], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("trackstub_without"), flags=("-ffp-contract=off",)))


A5 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)                               # int64 of 0xA5 bytes
PAD = 4


class Maps:
    """a caller's "device" buffers on the stand-in: host memory; the sums pre-filled with 0xA5 with 0xA5 words around them"""
    def __init__(self, s, disp, depth, normal, mask=None, conf=None):
        self.disp, self.depth, self.normal = (np.ascontiguousarray(a, np.float32) for a in (disp, depth, normal))
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.conf = None if conf is None else np.ascontiguousarray(conf, np.uint16)
        self.frames = s.frames
        self.out = np.full(29 * s.frames + 2 * PAD, A5, np.int64)

    sums_ptr = property(lambda self: self.out.ctypes.data + 8 * PAD)
    ptr = staticmethod(lambda a: None if a is None else a.ctypes.data)

    def untouched(self):
        return bool(np.all(self.out == A5))

    def sums(self):
        assert np.all(self.out[:PAD] == A5) and np.all(self.out[PAD + 29 * self.frames:] == A5)
        return self.out[PAD:PAD + 29 * self.frames].reshape(self.frames, 29)


def sums_call(L, inst, cs, cm, poses, b, **kw):
    a = dict(disp=b.ptr(b.disp), mask=b.ptr(b.mask), conf=b.ptr(b.conf), depth=b.ptr(b.depth), normal=b.ptr(b.normal), sums=b.sums_ptr)
    a.update(kw)
    return L.sgm_track_sums(inst, None if cs is None else C.byref(cs), None if cm is None else C.byref(cm),
                            None if poses is None else poses.ctypes.data, a["disp"], a["mask"], a["conf"], a["depth"], a["normal"], a["sums"])


def track_call(L, inst, cs, cm, poses, b, trace=True):
    """sgm_track on the stand-in: (ok, poses, stats, trace_sums, trace_poses)"""
    import soc_project_stereo_matching_amd as S
    poses = np.array(poses, np.float64).reshape(b.frames, 12)
    stats = (S.SGMTrackStats * b.frames)()
    n = cm.iterations
    t_sums, t_poses = np.zeros((n, b.frames, 29), np.int64), np.zeros((n + 1, b.frames, 12), np.float64)
    ok = L.sgm_track(inst, C.byref(cs), C.byref(cm), poses.ctypes.data, b.ptr(b.disp), b.ptr(b.mask), b.ptr(b.conf), b.ptr(b.depth),
                     b.ptr(b.normal), C.addressof(stats), t_sums.ctypes.data if trace else None, t_poses.ctypes.data if trace else None)
    return ok, poses, [dict(pixels=st.pixels, rms=st.rms, status=st.status) for st in stats], t_sums, t_poses


def test_the_validated_specs_the_poses_and_the_callers_pointers_arrive(host):
    L = host
    inst = L.sgm_create(0)                                        # never initialised: tracking needs no shape
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    b = Maps(s, disp, depth, normal, mask, conf)
    L.stub_clear(); L.stub_track_clear()
    assert sums_call(L, inst, c_source(s), c_model(m), poses, b)
    assert L.stub_track_count() == 1 and standin.log(L) == []     # no scratch, no copy, no wait without a match in flight
    assert [L.stub_track_ptr(0, k) for k in range(7)] == [b.disp.ctypes.data, b.mask.ctypes.data, b.conf.ctypes.data, b.depth.ctypes.data,
                                                          b.normal.ctypes.data, b.sums_ptr, poses.ctypes.data]
    assert np.array_equal(np.ctypeslib.as_array(L.stub_track_poses(0), (36,)), poses.reshape(-1))
    c, t = L.stub_track_source(0).contents, L.stub_track_model(0).contents
    assert (c.W, c.H, c.B, c.min_conf) == (s.width, s.height, s.frames, s.min_conf) and np.float32(c.fb) == CR.fb_of(s)
    assert (t.W, t.H) == (m.width, m.height) and [np.float32(x) for x in (t.fx, t.fy, t.cx, t.cy, t.dist_max, t.span)] == \
        [np.float32(x) for x in (m.fx, m.fy, m.cx, m.cy, m.dist_max, m.span)]
    assert b.sums().tolist() == TR.sums(disp, s, m, poses, depth, normal, mask, conf).tolist()
    L.sgm_destroy(inst)


@pytest.mark.parametrize("name", sorted(PLANTED_PIXELS))
def test_the_stand_in_agrees_on_the_planted_pixels(host, name):
    L = host
    inst = L.sgm_create(0)
    s, disp, m, poses, depth, normal = PLANTED_PIXELS[name]()
    b = Maps(s, disp, depth, normal)
    assert sums_call(L, inst, c_source(s), c_model(m), poses, b)
    assert b.sums().tolist() == TR.sums(disp, s, m, poses, depth, normal).tolist()
    L.sgm_destroy(inst)


def test_sgm_track_on_the_stand_in_equals_the_restatement_round_by_round(host):
    """the corner (converging), a frame that associates nothing (status 1 in round 0) and a single plane (status 2), in one batch:
    the failed frames sit out and keep their pose"""
    L = host
    inst = L.sgm_create(0)
    s, disp, m, depth, normal, true = corner_scene(4, frames=3)
    disp, depth, normal = disp.copy(), depth.copy(), normal.copy()
    disp[1] = INF
    depth[2], normal[2] = 2.0, (0.0, 0.0, -1.0)
    disp[2] = 20.0
    guess = np.stack([IDENTITY, pose_of(rodrigues((0.1, 0, 0)), (0, 0.1, 0)), IDENTITY])
    b = Maps(s, disp, depth, normal)
    L.stub_clear(); L.stub_track_clear()
    ok, poses, stats, t_sums, t_poses = track_call(L, inst, c_source(s), c_model(m), guess, b)
    assert ok and L.stub_track_count() == 4
    w_poses, w_stats, w_sums, w_trace = TR.track(disp, s, m, guess, depth, normal)
    assert [st["status"] for st in w_stats] == [0, 1, 2] and w_stats[2]["pixels"] > 1000
    assert stats == w_stats and poses.tobytes() == w_poses.tobytes()
    assert t_sums.tobytes() == w_sums.tobytes() and t_poses.tobytes() == w_trace.tobytes()
    assert t_poses[4, 1].tobytes() == guess[1].tobytes() and t_poses[4, 2].tobytes() == guess[2].tobytes()
    # the kernel received the poses rounded once to float32
    assert np.array_equal(np.ctypeslib.as_array(L.stub_track_poses(3), (36,)), t_poses[3].astype(np.float32).reshape(-1))
    names = [e.name for e in standin.log(L)]
    assert names.count("alloc") == 1 and names.count("d2h") == 4
    # without traces; the scratch is reserved once
    L.stub_clear()
    ok, poses2, stats2, _, _ = track_call(L, inst, c_source(s), c_model(m), guess, b, trace=False)
    assert ok and poses2.tobytes() == w_poses.tobytes() and stats2 == w_stats and "alloc" not in [e.name for e in standin.log(L)]
    L.sgm_destroy(inst)


def test_a_refused_allocation_fails_sgm_track_before_anything_is_queued(host, capfd):
    """the one buffer tracking reserves: sgm_track's own sums"""
    L = host
    inst = L.sgm_create(0)
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    L.stub_clear(); L.stub_track_clear()
    L.stub_fail_at(b"alloc", 0)
    ok, got, _, _, _ = track_call(L, inst, c_source(s), c_model(m), poses.astype(np.float64), Maps(s, disp, depth, normal))
    assert not ok and L.stub_track_count() == 0 and got.tobytes() == poses.astype(np.float64).tobytes()
    assert "device allocation failed for the sums of tracking" in capfd.readouterr().err
    assert "d2h" not in [e.name for e in standin.log(L)]
    L.sgm_destroy(inst)


def refused(L, inst, cs, cm, poses, b, capfd, entry="sgm_track_sums", **kw):
    capfd.readouterr()
    L.stub_clear(); L.stub_track_clear()
    assert not sums_call(L, inst, cs, cm, poses, b, **kw)
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("sgm_mi355x: " + entry), err
    assert L.stub_track_count() == 0 and standin.log(L) == [] and b.untouched()
    return err


MODEL_REFUSALS = dict(width=(0, 65536), height=(0, 65536), fx=(0.0, NAN, INF), fy=(-1.0,), cx=(INF,), cy=(NAN,), dist_max=(0.0, INF, NAN),
                      span=(0.0, -1.0, INF), iterations=(0, 65), min_pixels=(5, 0), min_pivot=(-0.5, NAN, INF))


def test_every_refusal(host, capfd):
    L = host
    inst = L.sgm_create(0)
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    b = Maps(s, disp, depth, normal, mask, conf)
    cs, cm = c_source(s), c_model(m)
    for field, values in MODEL_REFUSALS.items():
        for v in values:
            bad = c_model(m)
            setattr(bad, field, v)
            assert "the model is outside its ranges" in refused(L, inst, cs, bad, poses, b, capfd), (field, v)
    for field, v in (("width", 0), ("frames", 0), ("fx", 0.0), ("z_max", 0.0), ("min_conf", 65536)):
        bad = c_source(s)
        setattr(bad, field, v)
        assert "the source spec is outside its ranges" in refused(L, inst, bad, cm, poses, b, capfd), field
    many = c_source(s)
    many.frames = 65
    assert "65 frames" in refused(L, inst, many, cm, np.zeros((65, 12), np.float32), b, capfd)
    large = c_source(s)
    large.width, large.height, large.frames = 4097, 4096, 1
    assert "2^24" in refused(L, inst, large, cm, poses, b, capfd)
    bad_pose = poses.copy()
    bad_pose[2, 7] = INF
    assert "entry 7 of the pose of frame 2" in refused(L, inst, cs, cm, bad_pose, b, capfd)
    for kw in (dict(depth=None), dict(normal=None), dict(sums=None)):
        assert "NULL argument" in refused(L, inst, cs, cm, poses, b, capfd, **kw)
    assert "NULL" in refused(L, inst, None, cm, poses, b, capfd) and "NULL" in refused(L, inst, cs, None, poses, b, capfd)
    assert "NULL" in refused(L, inst, cs, cm, None, b, capfd)
    capfd.readouterr()
    assert not sums_call(L, None, cs, cm, poses, b) and "NULL" in capfd.readouterr().err
    for kw in (dict(sums=b.sums_ptr + 4), dict(disp=b.disp.ctypes.data + 2), dict(conf=b.conf.ctypes.data + 1), dict(depth=b.depth.ctypes.data + 1),
               dict(normal=b.normal.ctypes.data + 2)):
        assert "not aligned" in refused(L, inst, cs, cm, poses, b, capfd, **kw)
    for name in ("disp", "mask", "conf", "depth", "normal"):
        assert "overlap" in refused(L, inst, cs, cm, poses, b, capfd, sums=getattr(b, name).ctypes.data & ~7)
    # no map given and no match to take one from
    assert "no map given" in refused(L, inst, cs, cm, poses, b, capfd, disp=None)
    # sgm_track: its own NULLs and a pose that is finite as a double but not as a float
    import soc_project_stereo_matching_amd as S
    stats = (S.SGMTrackStats * s.frames)()
    p64 = poses.astype(np.float64)
    args = lambda **kw: [kw.get("p", p64.ctypes.data), b.disp.ctypes.data, None, None, b.depth.ctypes.data, b.normal.ctypes.data,
                         kw.get("stats", C.addressof(stats)), None, None]
    L.stub_clear(); L.stub_track_clear(); capfd.readouterr()
    assert not L.sgm_track(inst, C.byref(cs), C.byref(cm), *args(p=None)) and not L.sgm_track(inst, C.byref(cs), C.byref(cm), *args(stats=None))
    huge = p64.copy()
    huge[1, 9] = 1e300
    assert not L.sgm_track(inst, C.byref(cs), C.byref(cm), *args(p=huge.ctypes.data))
    err = capfd.readouterr().err
    assert err.count("sgm_mi355x: sgm_track:") == 3 and "entry 9 of the pose of frame 1" in err
    assert L.stub_track_count() == 0 and standin.log(L) == []
    assert L.sgm_track(inst, C.byref(cs), C.byref(cm), *args()) and L.stub_track_count() == 1
    L.sgm_destroy(inst)


def test_host_without_the_launcher_links_and_refuses(host_without, capfd):
    L = host_without
    inst = L.sgm_create(0)
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    b = Maps(s, disp, depth, normal)
    L.stub_clear(); capfd.readouterr()
    assert not sums_call(L, inst, c_source(s), c_model(m), poses, b)
    ok, _, _, _, _ = track_call(L, inst, c_source(s), c_model(m), poses.astype(np.float64), b)
    assert not ok
    assert capfd.readouterr().err.count("tracking is not part of this build") == 2 and standin.log(L) == [] and b.untouched()
    # the host-only entry points need no launcher
    m2, sums29 = corner_sums()
    out, st = np.empty(12), (C.c_byte * 16)()
    cm = c_model(m2)
    assert L.sgm_track_solve(C.byref(cm), sums29.ctypes.data, IDENTITY.ctypes.data, out.ctypes.data, C.addressof(st))
    assert out.tobytes() == np.array(TR.solve(m2, sums29, IDENTITY)[0]).tobytes()
    L.sgm_destroy(inst)


def test_a_refused_launch_fails_the_calls_and_a_call_waits_for_a_match_in_flight(host):
    L = host
    inst = L.sgm_create(0)
    s, disp, m, poses, depth, normal, mask, conf = noisy_case()
    b = Maps(s, disp, depth, normal)
    L.stub_track_clear()
    L.stub_track_fail_at(0)
    assert not sums_call(L, inst, c_source(s), c_model(m), poses, b) and L.stub_track_count() == 1 and b.untouched()
    L.stub_track_fail_at(1)
    cm = c_model(m)
    cm.iterations = 3
    ok, _, _, _, _ = track_call(L, inst, c_source(s), cm, poses.astype(np.float64), b)
    assert not ok and L.stub_track_count() == 3
    # behind a match whose post pass runs on a stream of its own: the call waits for the result's event
    import soc_project_stereo_matching_amd as S
    w, h = 24, 16
    opt = S.default_option(16)
    assert L.sgm_set_overlap_post(inst, 1) and L.sgm_initialize(inst, w, h, C.byref(opt))
    img = np.zeros((2, h, w), np.uint8)
    out = np.zeros((h, w), np.float32)
    assert L.sgm_match_device(inst, img[0].ctypes.data, img[1].ctypes.data, out.ctypes.data)
    one = CR.spec(w, h, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=1.0, doffs=1.0)
    b1 = Maps(one, out, depth[0], normal[0])
    L.stub_clear(); L.stub_track_clear()
    assert sums_call(L, inst, c_source(one), c_model(m), poses[:1], b1) and L.stub_track_count() == 1
    assert "wait_event" in [e.name for e in standin.log(L)] and "alloc" not in [e.name for e in standin.log(L)]
    L.sgm_destroy(inst)


# ---- the kernel's resources ----------------------------------------------------------------------------------------------------

def test_the_kernel_compiles_without_scratch_and_the_committed_table_is_this_builds(tmp_path):
    """the compile-time gate: the 29 int64 accumulators stay in registers -- 0 bytes of scratch and no spills in both
    instantiations -- and profiles/track_resources.txt records this build"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", fh.read(), re.M | re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sgm_track.hip"),
                          "-o", str(tmp_path / "sgm_track.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for block in out.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        num = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))
        assert "sgm_track_sums_k" in name, name
        got["sgm_track_sums_k<4>" if "ILi4E" in name else "sgm_track_sums_k<1>"] = [
            num(r"TotalSGPRs"), num(r" VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"),
            num(r"Occupancy \[waves/SIMD\]"), num(r"SGPRs Spill"), num(r"VGPRs Spill")]
    assert sorted(got) == ["sgm_track_sums_k<1>", "sgm_track_sums_k<4>"], got
    for name, (sgpr, vgpr, scratch, lds, occ, s_spill, v_spill) in got.items():
        assert scratch == 0 and s_spill == 0 and v_spill == 0 and vgpr >= 58, (name, got[name])
    with open(os.path.join(ROOT, "profiles", "track_resources.txt")) as fh:
        rows = [ln.split() for ln in fh.read().splitlines() if ln.startswith("sgm_track_sums_k<")]
    # kernel | SGPR VGPR scratch LDS occ. spills
    table = {r[0]: [int(x) for x in r[2:7]] + [int(x) for x in r[7].split("+")] for r in rows}
    assert table == got


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_track_host_is_asan_ubsan_clean(tmp_path):
    """tests/track_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in launcher."""
    exe = standin.build(tmp_path, sanitize=True, exe="track_sanitize_driver", flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "track_sanitize_driver.c"), STUB_TRACK])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("track_sanitize_driver ok")
