"""The TSDF volume ray-cast into depth and normal maps (extension; the contract is in include/sgm_mi355x.h, sgm_raycast_spec) without
a GPU: the numpy restatement tests/raycast_ref.py against a plain per-pixel Python loop with every operation rounded to float32, the
scenes of tests/test_volume_cpu.py rendered back, planted volumes of a few voxels with one ray each for every decision of the
contract, header / library / Python agreement, the C host's logic on the stand-in device (tests/stub_device.c + tests/stub_volume.c
+ tests/stub_raycast.c) and a sanitizer run of a stand-alone driver.  Tolerance 0 wherever the stand-in is compared with the
restatement."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as RR
import standin
import volume_ref as VR
from conftest import ROOT
from test_cloud_cpu import f32, div32
from test_volume_cpu import DeviceVolume, STUB_VOLUME, bad_volume, c_volume, moving_rig, noisy_scene, plane_scene, rot, small_scene

STUB_RAYCAST = os.path.join(ROOT, "tests", "stub_raycast.c")
_p, _i, _b = C.c_void_p, C.c_int, C.c_bool
INF, NAN = float("inf"), float("nan")
QNAN_BITS = 0x7FC00000


# ---- views and scenes (shared with tests/test_gpu_raycast.py) ------------------------------------------------------------------

def scene_view(w, h, frames=1, z_min=0.3, z_max=1.6, step=0.1, min_weight=1):
    """the view of the scenes' camera scaled to w x h: the field of view of the design's 70-pixel camera with fx = 40"""
    fx = 40.0 * w / 70.0
    return RR.view(w, h, fx, fx, (w - 1) / 2.0, (h - 1) / 2.0, z_min, z_max, step, min_weight, frames)


def c_view(vw):
    import soc_project_stereo_matching_amd as S
    return S.raycast_spec(vw.width, vw.height, vw.fx, vw.fy, vw.cx, vw.cy, vw.z_min, vw.z_max, vw.step, vw.min_weight, vw.frames)


@functools.lru_cache(maxsize=None)
def plane_volume():
    v, s, poses, disp = plane_scene()
    vox = VR.integrate(VR.empty(v), v, s, poses, disp)[0]
    vox.setflags(write=False)
    return v, vox


@functools.lru_cache(maxsize=None)
def noisy_volume():
    v, s, poses, disp = noisy_scene()
    vox = VR.integrate(VR.empty(v), v, s, poses, disp)[0]
    vox.setflags(write=False)
    return v, vox


def noisy_poses():
    """the moving rig's first two poses and a view rotated by 0.2 rad about y"""
    return np.concatenate([moving_rig(2), VR.pose(rot(1, 0.2), (0.25, -0.05, 0.1))[None]])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_maps(label, got, want):
    """depth or normal maps, bit for bit"""
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError(f"{label}: {len(bad)} of {g.size} values differ, first at {bad[0]}: {g[bad[0]]:#010x} != {w[bad[0]]:#010x}")


# ---- the restatement against a plain loop --------------------------------------------------------------------------------------

def loop_raycast(vox, v, vw, poses):
    """The definition of include/sgm_mi355x.h as a loop over Python floats: sums, products, quotients and square roots of float32
    values are exact or correctly rounded in double, so rounding each to float32 once is the float32 operation."""
    n = (v.nx, v.ny, v.nz)
    words = np.asarray(vox, np.uint32).reshape(v.nz, v.ny, v.nx)
    fx, fy, cx, cy, z_min, z_max, step, voxel = (float(np.float32(t)) for t in (vw.fx, vw.fy, vw.cx, vw.cy, vw.z_min, vw.z_max, vw.step, v.voxel))
    origin = [float(np.float32(o)) for o in v.origin]
    nan = float(np.array([QNAN_BITS], np.uint32).view(np.float32)[0])
    depth = np.empty((vw.frames, vw.height, vw.width), np.float32)
    normal = np.empty((vw.frames, vw.height, vw.width, 3), np.float32)

    def word(i, j, k):
        t = int(words[k, j, i])
        return (t & 0xFFFF) - (0x10000 if t & 0x8000 else 0), t >> 16

    def nearest(g):
        for a in range(3):
            if not math.isfinite(g[a]) or not 0.0 <= g[a] < float(n[a]):
                return 0
        tq, w = word(*(math.floor(t) for t in g))
        return 0 if w < vw.min_weight else (2 if tq < 0 else 1)

    def lerp(p, q, s):
        return f32(p + f32(s * f32(q - p)))

    def trilinear(g):
        i0, fr = [], []
        for a in range(3):
            h = f32(g[a] - 0.5)
            if not math.isfinite(h):
                return None
            lo = math.floor(h)
            if not (0 <= lo and f32(float(lo) + 1.0) < float(n[a])):
                return None
            i0.append(lo)
            fr.append(f32(h - float(lo)))
        t = {}
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    tq, w = word(i0[0] + dx, i0[1] + dy, i0[2] + dz)
                    if w < vw.min_weight:
                        return None
                    t[dx, dy, dz] = float(tq)
        c = [lerp(lerp(t[0, 0, dz], t[1, 0, dz], fr[0]), lerp(t[0, 1, dz], t[1, 1, dz], fr[0]), fr[1]) for dz in (0, 1)]
        return lerp(c[0], c[1], fr[2])

    for fr in range(vw.frames):
        P = [float(x) for x in np.asarray(poses, np.float32).reshape(-1, 12)[fr]]
        c = [-f32(f32(f32(P[i] * P[9]) + f32(P[3 + i] * P[10])) + f32(P[6 + i] * P[11])) for i in range(3)]
        for y in range(vw.height):
            for x in range(vw.width):
                a, b = div32(f32(float(x) - cx), fx), div32(f32(float(y) - cy), fy)
                d = [f32(f32(f32(P[i] * a) + f32(P[3 + i] * b)) + P[6 + i]) for i in range(3)]
                go = [div32(f32(c[i] - origin[i]), voxel) for i in range(3)]
                gd = [div32(d[i], voxel) for i in range(3)]
                at = lambda Z: [f32(go[i] + f32(Z * gd[i])) for i in range(3)]
                Zs, nrm = nan, [nan] * 3
                prev, Zp, Zc, front, k = 0, 0.0, 0.0, False, 0
                while True:
                    Zc = f32(z_min + f32(float(k) * step))
                    if not Zc <= z_max:
                        break
                    cur = nearest(at(Zc))
                    if prev == 1 and cur == 2:
                        front = True
                        break
                    if prev == 2 and cur == 1:
                        break
                    prev, Zp, k = cur, Zc, k + 1
                if front:
                    Fp, Fc = trilinear(at(Zp)), trilinear(at(Zc))
                    if Fp is not None and Fc is not None and f32(Fp - Fc) > 0:
                        s = min(max(div32(Fp, f32(Fp - Fc)), 0.0), 1.0)
                        Zs = f32(Zp + f32(s * step))
                        g = at(Zs)
                        nw = []
                        for ax in range(3):
                            up = trilinear([f32(g[i] + 1.0) if i == ax else g[i] for i in range(3)])
                            dn = trilinear([f32(g[i] - 1.0) if i == ax else g[i] for i in range(3)])
                            nw.append(None if up is None or dn is None else f32(up - dn))
                        if None not in nw:
                            m = [f32(f32(f32(P[3 * r] * nw[0]) + f32(P[3 * r + 1] * nw[1])) + f32(P[3 * r + 2] * nw[2])) for r in range(3)]
                            sq = f32(f32(f32(m[0] * m[0]) + f32(m[1] * m[1])) + f32(m[2] * m[2]))
                            length = f32(math.sqrt(sq)) if math.isfinite(sq) else sq
                            if math.isfinite(length) and length > 0:
                                nrm = [div32(t, length) for t in m]
                depth[fr, y, x] = Zs
                normal[fr, y, x] = nrm
    return depth, normal


def test_restatement_equals_the_loop():
    v, s, poses, disp, _, _ = small_scene()
    vox, _ = VR.integrate(VR.empty(v), v, s, poses, disp)
    vw = scene_view(13, 9, frames=2, z_min=0.4, z_max=1.7, step=0.07)
    cams = np.stack([VR.pose(), VR.pose(rot(1, 0.2), (0.25, -0.05, 0.1))])
    depth, normal, stats = RR.raycast(vox, v, vw, cams)
    want_d, want_n = loop_raycast(vox, v, vw, cams)
    same_maps("depth", depth, want_d)
    same_maps("normal", normal, want_n)
    assert stats["hits"] == int(np.isfinite(depth).sum()) > 20 and stats["normals"] == int(np.isfinite(normal[..., 0]).sum())
    # on the design's noisy volume too, a coarse view from the rotated camera: back faces and failed refinements included
    v, vox = noisy_volume()
    vw = scene_view(20, 12)
    depth, normal, stats = RR.raycast(vox, v, vw, noisy_poses()[2:])
    want_d, want_n = loop_raycast(vox, v, vw, noisy_poses()[2:])
    same_maps("noisy depth", depth, want_d)
    same_maps("noisy normal", normal, want_n)
    assert stats["hits"] > 50 and stats["refine_failed"] > 0


# ---- the scenes of the design --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,hits,failed,normals", [((70, 33), 1856, 322, 1728), ((24, 16), 220, 44, 220)])
def test_plane_scene_rendered_from_the_identity_pose(size, hits, failed, normals):
    v, vox = plane_volume()
    vw = scene_view(*size)
    depth, normal, stats = RR.raycast(vox, v, vw, VR.pose()[None])
    hit = np.isfinite(depth[0])
    assert stats == dict(hits=hits, back=0, refine_failed=failed, normals=normals) and hit.sum() == hits
    err = float(np.abs(depth[0][hit].astype(np.float64) - 1.03).max()) / v.voxel
    print("plane %dx%d: %d hits, max |Z - 1.03| = %.3g voxel" % (*size, hits, err))
    assert err <= 5e-4                                            # the bound of test_plane_scene_gives_the_plane
    assert hits > 0.5 * vw.width * vw.height
    ok = np.isfinite(normal[0][..., 0])
    assert ok.sum() == normals and not np.any(ok & ~hit)
    assert np.all(normal[0][ok] == np.array([0.0, 0.0, -1.0], np.float32))
    assert np.all(bits(depth[0][~hit]) == QNAN_BITS) and np.all(bits(normal[0][~ok]) == QNAN_BITS)
    # border pixels are empty: their rays meet the surface where the eight voxels are not all observed
    assert not hit[0].any() and not hit[-1].any() and not hit[:, 0].any() and not hit[:, -1].any()


def test_noisy_scene_covers_every_outcome():
    v, vox = noisy_volume()
    vw = scene_view(40, 24, frames=3)
    depth, normal, stats = RR.raycast(vox, v, vw, noisy_poses())
    print("noisy: %r" % stats)
    hit, ok = np.isfinite(depth), np.isfinite(normal[..., 0])
    assert stats["hits"] == hit.sum() > 1000 and stats["back"] >= 1 and stats["refine_failed"] >= 1
    assert (hit & ~ok).sum() >= 1 and stats["normals"] == ok.sum() > 500                      # depth without a normal
    n = normal[ok].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6) and (n[:, 2] < 0).mean() > 0.95
    assert np.all(np.abs(depth[hit].astype(np.float64) - 1.03) < 0.45)
    # one call over three frames is three calls of one frame
    for f in range(3):
        one = scene_view(40, 24)
        d1, n1, _ = RR.raycast(vox, v, one, noisy_poses()[f:f + 1])
        same_maps(f"frame {f}", d1[0], depth[f])
        same_maps(f"frame {f} normal", n1[0], normal[f])


# ---- planted volumes, one ray each ---------------------------------------------------------------------------------------------

def planted(columns, weights=None, at=(2.5, 2.5, 0.5), n_xy=5, z_min=1.0, z_max=None, step=1.0, min_weight=1):
    """(v, vox, view, poses) of a volume of n_xy x n_xy x len(tq) voxels of edge 1 and ONE ray along +z: with the identity pose and
    fx = fy = 1, cx = cy = 0 the pixel (0, 0) has a = b = 0, so g(Z) = (at_x, at_y, at_z - z_min + Z) exactly.  columns: {(i, j) or
    None: [tq of k = 0 ..]}, None for every column not named; weights alike (default 1)."""
    nz = len(columns[None])
    tq = np.zeros((nz, n_xy, n_xy), np.int64)
    w = np.ones((nz, n_xy, n_xy), np.int64)
    for src, dst in ((columns, tq), (weights or {}, w)):
        if None in src:
            dst[:] = np.asarray(src[None]).reshape(nz, 1, 1)
        for key, col in src.items():
            if key is not None:
                dst[:, key[1], key[0]] = col
    v = VR.spec(n_xy, n_xy, nz, 1.0, (-at[0], -at[1], z_min - at[2]), 0.25)
    vw = RR.view(1, 1, 1.0, 1.0, 0.0, 0.0, z_min, z_min + (nz - 1) * step if z_max is None else z_max, step, min_weight)
    return v, VR.pack(tq, w), vw, VR.pose()[None]


def near(x, towards):
    return float(np.nextafter(np.float32(x), np.float32(towards)))


# name -> (planted(..), depth or None, what the normal is: "z" (0, 0, -1), None (three NaNs), stats)
HIT, FAILED, BACK, MISS = (dict(hits=1, back=0, refine_failed=0), dict(hits=0, back=0, refine_failed=1), dict(hits=0, back=1, refine_failed=0),
                           dict(hits=0, back=0, refine_failed=0))
MIX = (2.25, 2.5, 0.5)                                            # h_x = 1.75: a quarter of column 1, three quarters of column 2
PLANTED_RAYS = {
    # tq == 0 counts as non-negative: as the previous sample it opens a front hit with s = 0, as the current one it is no hit ...
    "zero previous": (lambda: planted({None: [5, 0, -5, -5, -5]}), 2.0, "z", HIT),
    "zero current": (lambda: planted({None: [5, 5, 0, -5, -5]}), 3.0, "z", HIT),
    "zero first": (lambda: planted({None: [0, -5, -5, -5]}), 1.0, None, HIT),
    # ... and behind a negative sample it is a back face
    "zero behind negative": (lambda: planted({None: [-5, 0, 5, -5, -5]}), None, None, BACK),
    "plain": (lambda: planted({None: [10, 10, 5, -15, -15, -15]}), 3.25, "z", HIT),
    # an invalid sample forgets the previous one: no hit there, a hit further on
    "invalid between": (lambda: planted({None: [5, 5, -5, -5]}, {None: [1, 0, 1, 1]}), None, None, MISS),
    "invalid between, hit later": (lambda: planted({None: [5, 5, -5, 5, 5, -5, -5]}, {None: [1, 0, 1, 0, 1, 1, 1]}), 5.5, None, HIT),
    "invalid forgets a negative": (lambda: planted({None: [-5, 5, 5, -5, -5]}, {None: [1, 0, 1, 1, 1]}), 3.5, None, HIT),
    # a ray that starts behind the surface: a back face, and the front face behind it is not looked for
    "starts behind": (lambda: planted({None: [-5, 5, 5, -5, -5]}), None, None, BACK),
    # den <= 0 with both trilinear values valid (the neighbouring column runs the other way)
    "den negative": (lambda: planted({None: [5, 1, -1, -5], (1, 2): [5, -32000, 32000, -5], (1, 3): [5, -32000, 32000, -5]}, at=MIX), None, None, FAILED),
    "den zero": (lambda: planted({None: [5, 1, -1, -5], (1, 2): [5, -3, 3, -5], (1, 3): [5, -3, 3, -5]}, at=MIX), None, None, FAILED),
    # s clamped: Fp < 0 < den gives 0, Fc > 0 gives 1
    "s below 0": (lambda: planted({None: [5, 1, -1, -5], (1, 2): [5, -100, -30000, -5], (1, 3): [5, -100, -30000, -5]}, at=MIX), 2.0, "any", HIT),
    "s above 1": (lambda: planted({None: [5, 1, -1, -5, -5], (1, 2): [5, 30000, 100, -5, -5], (1, 3): [5, 30000, 100, -5, -5]}, at=MIX, z_max=4.0),
                  3.0, "any", HIT),
    # the trilinear cell leaves the grid on each of the six sides
    "cell leaves at x = 0": (lambda: planted({None: [5, 5, -5, -5]}, at=(0.25, 2.5, 0.5)), None, None, FAILED),
    "cell leaves at x = n": (lambda: planted({None: [5, 5, -5, -5]}, at=(4.75, 2.5, 0.5)), None, None, FAILED),
    "cell leaves at y = 0": (lambda: planted({None: [5, 5, -5, -5]}, at=(2.5, 0.25, 0.5)), None, None, FAILED),
    "cell leaves at y = n": (lambda: planted({None: [5, 5, -5, -5]}, at=(2.5, 4.75, 0.5)), None, None, FAILED),
    "cell leaves at z = 0": (lambda: planted({None: [5, -5, -5, -5]}, at=(2.5, 2.5, 0.25)), None, None, FAILED),
    "cell leaves at z = n": (lambda: planted({None: [5, 5, 5, -5]}, at=(2.5, 2.5, 0.75)), None, None, FAILED),
    "cell just inside": (lambda: planted({None: [5, 5, -5, -5]}, at=(0.5, 3.75, 0.5)), 2.5, None, HIT),
    # one of the eight words under min_weight
    "a word under min_weight": (lambda: planted({None: [5, 5, -5, -5]}, {None: [3, 3, 3, 3], (1, 3): [3, 3, 2, 3]}, at=MIX, min_weight=3), None, None, FAILED),
    "the words at min_weight": (lambda: planted({None: [5, 5, -5, -5]}, {None: [3, 3, 3, 3]}, at=MIX, min_weight=3), 2.5, "z", HIT),
    # a normal with one of its six samples invalid: the depth stays
    "normal misses a sample": (lambda: planted({None: [5, 5, -5, -5]}, {None: [1, 1, 1, 1], (4, 3): [1, 1, 0, 1]}), 2.5, None, HIT),
    # len == 0: the march starts at voxel 1, F(g* + e_z) == F(g* - e_z) == -7.5
    "normal of length 0": (lambda: planted({None: [-20, 5, -5, -10]}, at=(2.5, 2.5, 1.5), z_max=3.0), 1.5, None, HIT),
    # Z_k exactly equal to z_max is taken, the next one is not
    "z_max taken": (lambda: planted({None: [5, 5, -5, -5]}, z_max=3.0), 2.5, "z", HIT),
    "z_max before the hit": (lambda: planted({None: [5, 5, -5, -5]}, z_max=near(3.0, 0.0)), None, None, MISS),
    # g exactly on a voxel face belongs to the upper voxel (column 1 is not observed: a hit is then a failed refinement) ...
    "on a face": (lambda: planted({None: [5, 5, -5, -5]}, {None: [1, 1, 1, 1], (1, 2): [0, 0, 0, 0]}, at=(2.0, 2.5, 0.5)), None, None, FAILED),
    "below a face": (lambda: planted({None: [5, 5, -5, -5]}, {None: [1, 1, 1, 1], (1, 2): [0, 0, 0, 0]}, at=(near(2.0, 0.0), 2.5, 0.5)), None, None, MISS),
    # ... and g exactly at n_i is outside
    "at n": (lambda: planted({None: [5, 5, -5, -5]}, at=(5.0, 2.5, 0.5)), None, None, MISS),
    "below n": (lambda: planted({None: [5, 5, -5, -5]}, at=(near(5.0, 0.0), 2.5, 0.5)), None, None, FAILED),
    "at 0": (lambda: planted({None: [5, 5, -5, -5]}, at=(2.5, 0.0, 0.5)), None, None, FAILED),
    "below 0": (lambda: planted({None: [5, 5, -5, -5]}, at=(2.5, near(0.0, -1.0), 0.5)), None, None, MISS),
}


@pytest.mark.parametrize("name", sorted(PLANTED_RAYS))
def test_planted_ray(name):
    make, want_depth, want_normal, want_stats = PLANTED_RAYS[name]
    v, vox, vw, poses = make()
    depth, normal, stats = RR.raycast(vox, v, vw, poses)
    loop_d, loop_n = loop_raycast(vox, v, vw, poses)
    same_maps(name, depth, loop_d)
    same_maps(name, normal, loop_n)
    assert {k: stats[k] for k in want_stats} == want_stats, stats
    if want_depth is None:
        assert bits(depth)[0, 0, 0] == QNAN_BITS and np.all(bits(normal) == QNAN_BITS)
    else:
        assert depth[0, 0, 0] == np.float32(want_depth)
        if want_normal == "z":
            assert normal[0, 0, 0].tolist() == [0.0, 0.0, -1.0] and stats["normals"] == 1
        elif want_normal is None:
            assert np.all(bits(normal) == QNAN_BITS) and stats["normals"] == 0
        else:
            assert np.all(np.isfinite(normal)) and normal[0, 0, 0, 2] < 0


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


FIELDS = ["width", "height", "frames", "fx", "fy", "cx", "cy", "z_min", "z_max", "step", "min_weight"]


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    assert "sgm_volume_raycast" in _declared_functions() and hasattr(lib, "sgm_volume_raycast") and hasattr(lib, "sgmd_volume_raycast")
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    block = text.split("ray-cast into depth and normal maps of any view")[1].split("sgm_raycast_spec;")[0]
    for line in ("c_i = -((R[0][i]*t0 + R[1][i]*t1) + R[2][i]*t2)", "a = ((float)x - cx) / fx,   b = ((float)y - cy) / fy",
                 "d_i  = (R[0][i]*a + R[1][i]*b) + R[2][i]", "go_i = (c_i - origin_i) / voxel,   gd_i = d_i / voxel", "g(Z)_i = go_i + Z * gd_i",
                 "Z_k = z_min + (float)k * step", "lerp(p, q, s) = p + s*(q - p)", "s = fminf(fmaxf(Fp / den, 0), 1);   Z* = Z_{k-1} + s * step",
                 "nw_a = F(g* + e_a) - F(g* - e_a)", "n_r  = (R[r][0]*nw_0 + R[r][1]*nw_1) + R[r][2]*nw_2", "len  = sqrtf((n_0*n_0 + n_1*n_1) + n_2*n_2)"):
        assert line in block, line
    for out in ("adaptive step lengths", "shading and colour", "pose estimation", "row tiles"):
        assert out in block.split("Not part of it:")[1], out
    # ray-casting left the volume's own list
    volume_block = text.split("sgm_volume_spec;")[0].split("fused into a TSDF volume")[1]
    assert "Not part of it: meshing" in volume_block and "sgm_volume_raycast below" in volume_block
    assert C.sizeof(S.SGMRaycastSpec) == 44
    assert [f[0] for f in S.SGMRaycastSpec._fields_] == FIELDS
    assert [getattr(S.SGMRaycastSpec, n).offset for n in FIELDS] == list(range(0, 44, 4))
    body = re.search(r"typedef struct \{([^}]*)\} sgm_raycast_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == FIELDS
    assert callable(getattr(S.SGMInstance, "volume_raycast", None)) and callable(S.raycast_spec)
    t = S.raycast_spec(70, 33, 40.0, 41.0, 34.5, 16.0, 0.3, 1.6, 0.1, 3, 2)
    assert (t.width, t.height, t.frames, t.fx, t.fy, t.cx, t.cy, t.min_weight) == (70, 33, 2, 40.0, 41.0, 34.5, 16.0, 3)
    assert (np.float32(t.z_min), np.float32(t.z_max), np.float32(t.step)) == (np.float32(0.3), np.float32(1.6), np.float32(0.1))


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

class DeviceView(C.Structure):                                   # sgmd_raycast of csrc/sgm_device.h
    _fields_ = [("W", _i), ("H", _i), ("B", _i)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "z_min", "z_max", "step")] + \
               [("min_weight", C.c_uint)]


def _sign(L):
    for name, (res, args) in {"sgm_volume_raycast": (_b, [_p] * 7), "stub_raycast_clear": (None, []), "stub_raycast_count": (_i, []),
                              "stub_raycast_ptr": (_p, [_i, _i]), "stub_raycast_volume": (C.POINTER(DeviceVolume), [_i]),
                              "stub_raycast_view": (C.POINTER(DeviceView), [_i]), "stub_raycast_poses": (C.POINTER(C.c_float), [_i]),
                              "stub_raycast_fail_at": (None, [_i]), "stub_volume_clear": (None, []), "stub_volume_count": (_i, []),
                              "sgm_volume_bytes": (C.c_size_t, [_p])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("raycaststub"), extra_sources=[STUB_VOLUME, STUB_RAYCAST], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    """the volume's launchers without the ray-cast's"""
    return _sign(standin.build(tmp_path_factory.mktemp("raycaststub_without"), extra_sources=[STUB_VOLUME], flags=("-ffp-contract=off",)))


W, H = 48, 20
A5 = 0xA5A5A5A5
PAD = 8                                                           # words of 0xA5 on either side of an output


class Outputs:
    """a caller's "device" buffers on the stand-in: host memory; the volume's words, depth and normals pre-filled with 0xA5 with
    0xA5 words around them"""
    def __init__(self, vox, vw):
        self.voxels = np.ascontiguousarray(vox, np.uint32).reshape(-1).copy()
        self.before = self.voxels.copy()
        self.px = vw.frames * vw.height * vw.width
        self.shape = (vw.frames, vw.height, vw.width)
        self.d = np.full(self.px + 2 * PAD, A5, np.uint32)
        self.n = np.full(3 * self.px + 2 * PAD, A5, np.uint32)

    depth_ptr = property(lambda self: self.d.ctypes.data + 4 * PAD)
    normal_ptr = property(lambda self: self.n.ctypes.data + 4 * PAD)

    def untouched(self):
        return bool(np.all(self.d == A5) and np.all(self.n == A5) and np.array_equal(self.voxels, self.before))

    def depth(self):
        assert np.all(self.d[:PAD] == A5) and np.all(self.d[PAD + self.px:] == A5) and np.array_equal(self.voxels, self.before)
        return self.d[PAD:PAD + self.px].view(np.float32).reshape(self.shape)

    def normal(self):
        assert np.all(self.n[:PAD] == A5) and np.all(self.n[PAD + 3 * self.px:] == A5)
        return self.n[PAD:PAD + 3 * self.px].view(np.float32).reshape(self.shape + (3,))


def raycast_call(L, s, cv, cw, poses, o, voxels="own", depth="own", normal="own"):
    return L.sgm_volume_raycast(s, None if cv is None else C.byref(cv), None if cw is None else C.byref(cw),
                                None if poses is None else poses.ctypes.data, o.voxels.ctypes.data if isinstance(voxels, str) else voxels,
                                o.depth_ptr if isinstance(depth, str) else depth, o.normal_ptr if isinstance(normal, str) else normal)


def good_view(frames=1, **kw):
    d = dict(w=24, h=16, frames=frames, z_min=0.3, z_max=1.6, step=0.1, min_weight=1)
    d.update(kw)
    return scene_view(d.pop("w"), d.pop("h"), **d)


def test_the_validated_specs_the_poses_and_the_callers_pointers_arrive(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: the ray-cast needs no shape
    v, vox = noisy_volume()
    vw = good_view(frames=3, min_weight=2)
    poses = noisy_poses()
    o = Outputs(vox, vw)
    cv, cw = c_volume(v), c_view(vw)
    L.stub_clear(); L.stub_volume_clear(); L.stub_raycast_clear()
    assert raycast_call(L, s, cv, cw, poses, o)
    assert L.stub_raycast_count() == 1 and L.stub_volume_count() == 0
    assert [L.stub_raycast_ptr(0, k) for k in range(4)] == [o.voxels.ctypes.data, o.depth_ptr, o.normal_ptr, poses.ctypes.data]
    assert np.array_equal(np.ctypeslib.as_array(L.stub_raycast_poses(0), (36,)), poses.reshape(-1))             # the poses as given
    assert bytes(L.stub_raycast_volume(0).contents) == bytes(cv) and bytes(L.stub_raycast_view(0).contents) == bytes(cw)
    assert standin.log(L) == []                                   # no scratch, no copy, no wait without a match in flight
    want_d, want_n, stats = RR.raycast(vox, v, vw, poses)
    assert stats["hits"] > 100
    same_maps("depth", o.depth(), want_d)
    same_maps("normal", o.normal(), want_n)
    # d_normal == NULL: the depth alone, nothing where normals would go
    o2 = Outputs(vox, vw)
    assert raycast_call(L, s, cv, cw, poses, o2, normal=None) and L.stub_raycast_ptr(1, 2) is None
    same_maps("depth without normals", o2.depth(), want_d)
    assert np.all(o2.n == A5) and standin.log(L) == []
    L.sgm_destroy(s)


@pytest.mark.parametrize("scene", ["plane 70x33", "plane 24x16", "noisy"])
def test_the_stand_in_equals_the_restatement(host, scene):
    L = host
    s = L.sgm_create(0)
    if scene == "noisy":
        (v, vox), vw, poses = noisy_volume(), scene_view(40, 24, frames=3), noisy_poses()
    else:
        (v, vox), vw, poses = plane_volume(), scene_view(*(int(t) for t in scene.split()[1].split("x"))), VR.pose()[None]
    o = Outputs(vox, vw)
    assert raycast_call(L, s, c_volume(v), c_view(vw), poses, o)
    want_d, want_n, stats = RR.raycast(vox, v, vw, poses)
    assert stats["hits"] > 200
    same_maps(scene + " depth", o.depth(), want_d)
    same_maps(scene + " normal", o.normal(), want_n)
    L.sgm_destroy(s)


def test_the_stand_in_agrees_on_the_planted_rays(host):
    L = host
    s = L.sgm_create(0)
    for name, (make, _, _, _) in sorted(PLANTED_RAYS.items()):
        v, vox, vw, poses = make()
        o = Outputs(vox, vw)
        assert raycast_call(L, s, c_volume(v), c_view(vw), poses, o), name
        want_d, want_n, _ = RR.raycast(vox, v, vw, poses)
        same_maps(name + " depth", o.depth(), want_d)
        same_maps(name + " normal", o.normal(), want_n)
    L.sgm_destroy(s)


VIEW_REFUSALS = {
    "width 0": dict(width=0), "width 65536": dict(width=65536), "height 0": dict(height=0), "height 65536": dict(height=65536),
    "frames 0": dict(frames=0), "frames 65": dict(frames=65), "frames*width*height > 2^31": dict(width=65535, height=65535, frames=1),
    "fx 0": dict(fx=0.0), "fx < 0": dict(fx=-1.0), "fx NaN": dict(fx=NAN), "fx INF": dict(fx=INF), "fy 0": dict(fy=0.0), "fy NaN": dict(fy=NAN),
    "fy INF": dict(fy=INF), "cx NaN": dict(cx=NAN), "cx INF": dict(cx=INF), "cy NaN": dict(cy=NAN), "cy -INF": dict(cy=-INF),
    "z_min NaN": dict(z_min=NAN), "z_min < 0": dict(z_min=-0.1), "z_max NaN": dict(z_max=NAN), "z_max INF": dict(z_max=INF),
    "z_max == z_min": dict(z_min=0.5, z_max=0.5), "z_max < z_min": dict(z_min=0.5, z_max=0.4),
    "step 0": dict(step=0.0), "step < 0": dict(step=-0.1), "step NaN": dict(step=NAN), "step INF": dict(step=INF),
    "65536 steps": dict(z_min=0.0, z_max=65536.0, step=1.0), "min_weight 0": dict(min_weight=0), "min_weight 65536": dict(min_weight=65536),
}


def refused(L, s, cv, cw, poses, o, capfd, **kw):
    """false, one line on stderr that names the entry point, nothing logged, the outputs untouched"""
    L.stub_clear(); L.stub_raycast_clear()
    capfd.readouterr()
    assert not raycast_call(L, s, cv, cw, poses, o, **kw)
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("sgm_mi355x: sgm_volume_raycast: "), err
    assert L.stub_raycast_count() == 0 and standin.log(L) == [] and o.untouched()
    return err


@pytest.mark.parametrize("name", sorted(VIEW_REFUSALS))
def test_every_refusal_of_the_view(host, capfd, name):
    L = host
    s = L.sgm_create(0)
    v, vox = plane_volume()
    vw = good_view()
    cw = c_view(vw)
    for field, value in VIEW_REFUSALS[name].items():
        setattr(cw, field, value)
    err = refused(L, s, c_volume(v), cw, moving_rig(max(1, min(cw.frames, 65))), Outputs(vox, vw), capfd)
    assert "the view is outside its ranges" in err
    L.sgm_destroy(s)


def test_the_largest_march_is_taken(host):
    L = host
    s = L.sgm_create(0)
    v, vox = plane_volume()
    step = np.float32(0.1)
    z_max = np.float32(65536.0 * float(step))
    while float(z_max) / float(step) >= 65536.0:                  # the largest z_max the host takes with this step
        z_max = np.nextafter(z_max, np.float32(0.0))
    vw = RR.view(2, 1, 40.0, 40.0, 0.5, 0.0, 0.0, float(z_max), float(step))
    cw = c_view(vw)
    cw.z_max = float(np.nextafter(z_max, np.float32(INF)))
    assert not raycast_call(L, s, c_volume(v), cw, VR.pose()[None], Outputs(vox, vw))
    o = Outputs(vox, vw)
    assert raycast_call(L, s, c_volume(v), c_view(vw), VR.pose()[None], o)
    want = RR.raycast(vox, v, vw, VR.pose()[None])[0]
    assert np.all(np.isfinite(want))
    same_maps("65535.99 steps", o.depth(), want)
    L.sgm_destroy(s)


def test_every_refusal_of_the_volume_spec(host, capfd):
    from test_volume_cpu import VOLUME_REFUSALS
    L = host
    s = L.sgm_create(0)
    v, vox = plane_volume()
    vw = good_view()
    for name, kw in sorted(VOLUME_REFUSALS.items()):
        err = refused(L, s, c_volume(bad_volume(**kw)), c_view(vw), VR.pose()[None], Outputs(vox, vw), capfd)
        assert "the volume spec is outside its ranges" in err, name
    L.sgm_destroy(s)


def test_64_frames_are_taken_and_a_non_finite_pose_entry_is_not(host, capfd):
    L = host
    s = L.sgm_create(0)
    v, vox = noisy_volume()
    vw = good_view(frames=64, w=12, h=8)
    poses = moving_rig(64)
    o = Outputs(vox, vw)
    assert raycast_call(L, s, c_volume(v), c_view(vw), poses, o)
    want_d, want_n, stats = RR.raycast(vox, v, vw, poses)
    assert stats["hits"] > 64 * 20
    same_maps("64 frames", o.depth(), want_d)
    same_maps("64 frames normal", o.normal(), want_n)
    o = Outputs(vox, vw)
    for at in (0, 5, 11, 12 * 63 + 11, 12 * 17 + 9):
        for bad in (NAN, INF, -INF):
            p = poses.copy()
            p.reshape(-1)[at] = bad
            assert "is not finite" in refused(L, s, c_volume(v), c_view(vw), p, o, capfd), (at, bad)
    L.sgm_destroy(s)


def test_null_overlap_and_misaligned_refusals(host, capfd):
    L = host
    s = L.sgm_create(0)
    v, vox = plane_volume()
    vw = good_view()
    cv, cw = c_volume(v), c_view(vw)
    poses = VR.pose()[None]
    o = Outputs(vox, vw)
    x, d, n = o.voxels.ctypes.data, o.depth_ptr, o.normal_ptr
    vol_bytes, depth_bytes = o.voxels.nbytes, 4 * o.px
    assert vol_bytes > 3 * depth_bytes
    nulls = [lambda: refused(L, None, cv, cw, poses, o, capfd), lambda: refused(L, s, None, cw, poses, o, capfd),
             lambda: refused(L, s, cv, None, poses, o, capfd), lambda: refused(L, s, cv, cw, None, o, capfd),
             lambda: refused(L, s, cv, cw, poses, o, capfd, voxels=None), lambda: refused(L, s, cv, cw, poses, o, capfd, depth=None)]
    for k, call in enumerate(nulls):
        assert "NULL argument" in call(), k
    for k, kw in enumerate((dict(voxels=x + 2), dict(voxels=x + 1), dict(depth=d + 2), dict(depth=d + 1), dict(normal=n + 2), dict(normal=n + 3))):
        assert "not aligned" in refused(L, s, cv, cw, poses, o, capfd, **kw), k
    # an output that overlaps the volume, from its first to its last byte, or the other output
    for k, kw in enumerate((dict(depth=x), dict(depth=x + vol_bytes - 4), dict(depth=x - depth_bytes + 4), dict(normal=x), dict(normal=x + vol_bytes - 4),
                            dict(normal=x - 3 * depth_bytes + 4), dict(normal=d), dict(normal=d + depth_bytes - 4), dict(normal=d - 3 * depth_bytes + 4),
                            dict(depth=n), dict(depth=n + 3 * depth_bytes - 4))):
        assert "overlaps" in refused(L, s, cv, cw, poses, o, capfd, **kw), k
    # allowed: outputs that touch -- the depth right behind the volume's last word, the normals right behind the depth
    both = np.full(o.px * 4 + 2 * PAD, A5, np.uint32)
    assert raycast_call(L, s, cv, cw, poses, o, depth=both.ctypes.data, normal=both.ctypes.data + depth_bytes)
    want_d, want_n, _ = RR.raycast(vox, v, vw, poses)
    same_maps("touching", both[:o.px].view(np.float32), want_d)
    same_maps("touching normal", both[o.px:4 * o.px].view(np.float32), want_n)
    assert np.all(both[4 * o.px:] == A5)
    L.sgm_destroy(s)


def test_host_without_the_launcher_links_and_refuses(host_without, capfd):
    L = host_without
    s = L.sgm_create(0)
    v, vox = plane_volume()
    vw = good_view()
    o = Outputs(vox, vw)
    L.stub_clear()
    capfd.readouterr()
    assert not raycast_call(L, s, c_volume(v), c_view(vw), VR.pose()[None], o)
    err = capfd.readouterr().err
    assert err == "sgm_mi355x: sgm_volume_raycast: the ray-cast is not part of this build\n"
    assert standin.log(L) == [] and o.untouched()
    assert L.sgm_volume_bytes(C.byref(c_volume(v))) == vox.nbytes     # the volume itself is still there
    L.sgm_destroy(s)


def test_plain_match_logs_what_it_logs_without_the_raycast(host, host_without):
    """allocations and their sizes included: an instance that never renders is the instance it was"""
    import soc_project_stereo_matching_amd as S
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs, launches = [], []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        if hasattr(L, "stub_raycast_clear"):
            L.stub_raycast_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                                           conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        launches.append(standin.launches(L))
        L.sgm_destroy(s)
    assert launches[0] == launches[1] and logs[0] == logs[1] and len(launches[0]) > 10
    assert host.stub_raycast_count() == 0


def test_a_refused_launch_or_wait_fails_the_call_and_the_call_waits_for_a_match_in_flight(host):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    opt = S.default_option(16)
    assert L.sgm_reset(s, W, H, C.byref(opt))
    v, vox = plane_volume()
    vw = good_view()
    cv, cw = c_volume(v), c_view(vw)
    poses = VR.pose()[None]
    o = Outputs(vox, vw)
    L.stub_raycast_clear()
    L.stub_raycast_fail_at(0)
    assert not raycast_call(L, s, cv, cw, poses, o) and L.stub_raycast_count() == 1 and o.untouched()
    assert raycast_call(L, s, cv, cw, poses, o) and np.isfinite(o.depth()).sum() == 220          # the instance goes on
    # with the post pass on a stream of its own the call waits for the result of a match that is still in flight
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    L.stub_clear()
    assert raycast_call(L, s, cv, cw, poses, o)
    assert "wait_event" in [e.name for e in standin.log(L)] and "alloc" not in [e.name for e in standin.log(L)]
    assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
    L.stub_clear()
    L.stub_fail_at(b"wait_event", 0)
    L.stub_raycast_clear()
    assert not raycast_call(L, s, cv, cw, poses, o) and L.stub_raycast_count() == 0
    assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_raycast_host_is_asan_ubsan_clean(tmp_path):
    """tests/raycast_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in launchers."""
    exe = standin.build(tmp_path, sanitize=True, exe="raycast_sanitize_driver",
                        flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "raycast_sanitize_driver.c"), STUB_VOLUME, STUB_RAYCAST])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("raycast_sanitize_driver ok")
