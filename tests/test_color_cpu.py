"""Colour in the TSDF volume (extension; the contract is the colour section of include/sgm_mi355x.h) without a GPU: the numpy
restatement tests/color_ref.py against plain Python loops, against the volume's and the ray-cast's restatements, the conditions the
scenes must meet for the device tests to be about something, header / library / Python agreement, the C host's logic and the
driver on the stand-in device (tests/stub_device.c + stub_volume.c + stub_raycast.c + stub_mesh.c + stub_color.c), a sanitizer run of
a stand-alone driver and the kernels' compile-time resources.  Tolerance 0 wherever the stand-in is compared with the restatement."""
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
import color_ref as KR
import mesh_ref as MR
import raycast_ref as RR
import standin
import volume_ref as VR
from conftest import ROOT
from test_cloud_cpu import f32, div32
from test_raycast_cpu import STUB_RAYCAST, DeviceView, c_view, same_maps, scene_view
from test_volume_cpu import (STUB_VOLUME, DeviceSrc, DeviceVolume, VOLUME_REFUSALS, bad_volume, c_source, c_volume, camera, moving_rig,
                             noisy_maps, small_scene)

STUB_COLOR = os.path.join(ROOT, "tests", "stub_color.c")
STUB_MESH = os.path.join(ROOT, "tests", "stub_mesh.c")
_p, _i, _b, _z = C.c_void_p, C.c_int, C.c_bool, C.c_size_t
NAN = float("nan")
A5 = 0xA5A5A5A5


# ---- scenes (shared with tests/test_gpu_volume_color.py) -----------------------------------------------------------------------

def images_of(s, rng, channels):
    """a random image registered to the maps of s: uint8 grey, or uint32 r | g << 8 | b << 16 with noise in the top byte"""
    shape = (s.frames, s.height, s.width)
    if channels == 1:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def planted_start(v, rng):
    """(voxels, colours) a call starts from: mostly empty; one voxel in ten with a history (w 1..3, a random colour of weight 1..3),
    one in twenty with a colour weight of 254 and one in twenty with 255"""
    shape = (v.nz, v.ny, v.nx)
    kind = rng.random(shape)
    tq, w = rng.integers(-20000, 20000, shape), rng.integers(1, 4, shape)
    vox = np.where(kind < 0.2, VR.pack(tq, w), 0).astype(np.uint32)
    cw = np.where(kind < 0.1, rng.integers(1, 4, shape), np.where(kind < 0.15, 254, np.where(kind < 0.2, 255, 0)))
    r, g, b = (rng.integers(0, 256, shape) for _ in range(3))
    col = np.where(cw > 0, KR.pack(r, g, b, cw), 0).astype(np.uint32)
    return vox, col


def slab_zeroed(v, col):
    """the colour weights of four planes of x taken away (the bytes of the colours stay): the rays that end in the slab hit a
    surface without colour, those that end beside it find no eight coloured words and fall back to the nearest"""
    out = np.array(col, np.uint32).reshape(v.nz, v.ny, v.nx).copy()
    out[:, :, v.nx // 2 - 2:v.nx // 2 + 2] &= np.uint32(0x00FFFFFF)
    return out


def invalid_ids(v, id_kinds):
    """ids of every kind, valid and not: every e of 0..id_kinds-1 (the last names no kind; with 4 that is e == 3) along the row through
    the middle of the volume, whose last voxel has its far voxel outside the grid; the top plane (dz leaves); n out of range"""
    total = v.nx * v.ny * v.nz
    row = ((v.nz // 2) * v.ny + v.ny // 2) * v.nx + np.arange(v.nx)
    top = ((v.nz - 1) * v.ny + v.ny // 2) * v.nx + np.arange(0, v.nx, 5)
    ids = [n * id_kinds + e for n in np.concatenate([row, top]) for e in range(id_kinds)]
    ids += [total * id_kinds, total * id_kinds + 1, (total + 7) * id_kinds + 2, 0xFFFFFFFF, 0xFFFFFFF8]
    return np.array(ids, np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def colored_scene():
    """(v, s, poses, disp, image, voxels, colours): the 36 x 33 x 20 volume of the design under three noisy frames of the moving rig
    with a four-channel image, from a planted start; max_weight above 255, so the colour weight is capped by its eight bits"""
    v = VR.spec(36, 33, 20, 0.05, (-0.9, -0.825, 0.5), 0.2, max_weight=1000)
    s = CR.spec(70, 33, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=1.0, frames=3)
    rng = np.random.default_rng(131)
    disp, image = noisy_maps(s, rng), images_of(s, rng, 4)
    vox, col = planted_start(v, rng)
    for a in (vox, col):                                          # (the maps go to the device as they are: they stay writable)
        a.setflags(write=False)
    return v, s, moving_rig(3), disp, image, vox, col


@functools.lru_cache(maxsize=None)
def painted_scene():
    """(v, voxels, colours, the colours with the slab zeroed) of the coloured scene after its three frames, by the restatement"""
    v, s, poses, disp, image, vox0, col0 = colored_scene()
    vox, col, _ = KR.integrate(vox0, col0, v, s, poses, disp, None, None, image, 4)
    slab = slab_zeroed(v, col)
    for a in (vox, col, slab):
        a.setflags(write=False)
    return v, vox, col, slab


# ---- the restatement against plain loops ---------------------------------------------------------------------------------------

def loop_integrate(vox, col, v, s, poses, disp, mask, conf, image, channels):
    """The colour section of include/sgm_mi355x.h (and, for the condition, the volume's) as a loop over voxels and Python floats:
    sums, products and quotients of two float32 values are exact or correctly rounded in double, so rounding each to float32 once is
    the float32 operation.  Returns (voxels, colours)."""
    fb = f32(float(np.float32(s.fx)) * float(np.float32(s.baseline)))
    fx, fy, cx, cy, doffs, z_min, z_max = (float(np.float32(x)) for x in (s.fx, s.fy, s.cx, s.cy, s.doffs, s.z_min, s.z_max))
    voxel, trunc = float(np.float32(v.voxel)), float(np.float32(v.trunc))
    o = [float(np.float32(x)) for x in v.origin]
    out = np.array(vox, np.uint32).reshape(v.nz, v.ny, v.nx).copy()
    cout = np.array(col, np.uint32).reshape(v.nz, v.ny, v.nx).copy()
    for k in range(v.nz):
        for j in range(v.ny):
            for i in range(v.nx):
                p = [f32(o[a] + f32(f32(float(n) + 0.5) * voxel)) for a, n in enumerate((i, j, k))]
                word, cword = int(out[k, j, i]), int(cout[k, j, i])
                tq, w = (word & 0xFFFF) - (0x10000 if word & 0x8000 else 0), word >> 16
                c, cw = [(cword >> sh) & 0xFF for sh in (0, 8, 16)], cword >> 24
                for fr in range(s.frames):
                    P = [float(x) for x in np.asarray(poses, np.float32).reshape(-1, 12)[fr]]
                    Xp, Yp, Zp = (f32(f32(f32(f32(P[3 * r] * p[0]) + f32(P[3 * r + 1] * p[1])) + f32(P[3 * r + 2] * p[2])) + P[9 + r])
                                  for r in range(3))
                    if not math.isfinite(Zp) or not Zp > 0:
                        continue
                    u, vv = f32(f32(fx * div32(Xp, Zp)) + cx), f32(f32(fy * div32(Yp, Zp)) + cy)
                    if not (math.isfinite(u) and math.isfinite(vv)):
                        continue
                    uf, vf = math.floor(f32(u + 0.5)), math.floor(f32(vv + 0.5))
                    if not (0 <= uf < s.width and 0 <= vf < s.height):
                        continue
                    d = float(disp[fr, vf, uf])
                    if not math.isfinite(d) or (mask is not None and mask[fr, vf, uf] == 0) or (conf is not None and int(conf[fr, vf, uf]) < s.min_conf):
                        continue
                    den = f32(d + doffs)
                    if not (math.isfinite(den) and den > 0):
                        continue
                    Z = div32(fb, den)
                    if not (math.isfinite(Z) and z_min <= Z <= z_max):
                        continue
                    sdf = f32(Z - Zp)
                    if sdf < -trunc:
                        continue
                    q = int(np.rint(np.float32(f32(div32(min(sdf, trunc), trunc) * 32767.0))))
                    num, den_i = tq * w + q, w + 1
                    tq = (2 * num + den_i) // (2 * den_i)
                    w = min(w + 1, v.max_weight)
                    if sdf <= trunc:
                        pix = int(image[fr, vf, uf])
                        px = [pix, pix, pix] if channels == 1 else [pix & 0xFF, (pix >> 8) & 0xFF, (pix >> 16) & 0xFF]
                        c = [(2 * (c[ch] * cw + px[ch]) + (cw + 1)) // (2 * (cw + 1)) for ch in range(3)]
                        cw = min(cw + 1, min(v.max_weight, 255))
                out[k, j, i] = (w << 16) | (tq & 0xFFFF)
                cout[k, j, i] = (cw << 24) | (c[2] << 16) | (c[1] << 8) | c[0]
    return out, cout


def _lerp32(p, q, s):
    return f32(p + f32(s * f32(q - p)))


def loop_pixel_color(col, v, g):
    """the colour at g* = g (three Python floats that are float32 values): trilinear, else nearest, else 0"""
    n = (v.nx, v.ny, v.nz)
    col = np.asarray(col, np.uint32).reshape(v.nz, v.ny, v.nx)
    h = [f32(t - 0.5) for t in g]
    if all(math.isfinite(t) for t in h):
        lo = [math.floor(t) for t in h]
        if all(0 <= lo[a] and f32(float(lo[a]) + 1.0) < float(n[a]) for a in range(3)):
            fr = [f32(h[a] - float(lo[a])) for a in range(3)]
            words = {(dx, dy, dz): int(col[lo[2] + dz, lo[1] + dy, lo[0] + dx]) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
            if all(t >> 24 for t in words.values()):
                out = 0xFF000000
                for sh in (0, 8, 16):
                    t = {key: float((word >> sh) & 0xFF) for key, word in words.items()}
                    c = [_lerp32(_lerp32(t[0, 0, dz], t[1, 0, dz], fr[0]), _lerp32(t[0, 1, dz], t[1, 1, dz], fr[0]), fr[1]) for dz in (0, 1)]
                    out |= int(np.rint(np.float32(min(max(_lerp32(c[0], c[1], fr[2]), 0.0), 255.0)))) << sh
                return out
    if not all(math.isfinite(t) and 0.0 <= t < float(n[a]) for a, t in enumerate(g)):
        return 0
    word = int(col[math.floor(g[2]), math.floor(g[1]), math.floor(g[0])])
    return (0xFF000000 | word) if word >> 24 else 0


def loop_raycast_colors(col, v, vw, poses, depth):
    """rgba of the hits of `depth` (the ray-cast's own restatement gave it), pixel by pixel"""
    fx, fy, cx, cy, voxel = (float(np.float32(t)) for t in (vw.fx, vw.fy, vw.cx, vw.cy, v.voxel))
    origin = [float(np.float32(t)) for t in v.origin]
    out = np.zeros(depth.shape, np.uint32)
    for fr in range(vw.frames):
        P = [float(x) for x in np.asarray(poses, np.float32).reshape(-1, 12)[fr]]
        c = [-f32(f32(f32(P[i] * P[9]) + f32(P[3 + i] * P[10])) + f32(P[6 + i] * P[11])) for i in range(3)]
        for y in range(vw.height):
            for x in range(vw.width):
                Z = float(depth[fr, y, x])
                if not math.isfinite(Z):
                    continue
                a, b = div32(f32(float(x) - cx), fx), div32(f32(float(y) - cy), fy)
                d = [f32(f32(f32(P[i] * a) + f32(P[3 + i] * b)) + P[6 + i]) for i in range(3)]
                g = [f32(div32(f32(c[i] - origin[i]), voxel) + f32(Z * div32(d[i], voxel))) for i in range(3)]
                out[fr, y, x] = loop_pixel_color(col, v, g)
    return out


def loop_colors(vox, col, v, ids, id_kinds):
    vox, col = np.asarray(vox, np.uint32).reshape(-1), np.asarray(col, np.uint32).reshape(-1)
    tq = lambda word: (int(word) & 0xFFFF) - (0x10000 if int(word) & 0x8000 else 0)
    out = []
    for rid in (int(t) for t in ids):
        n, e = rid // id_kinds, rid % id_kinds
        out.append(0)
        if n >= vox.size or e >= id_kinds - 1:
            continue
        i, j, k = n % v.nx, (n // v.nx) % v.ny, n // (v.nx * v.ny)
        dx, dy, dz = MR.KINDS[e]
        if i + dx >= v.nx or j + dy >= v.ny or k + dz >= v.nz:
            continue
        m = ((k + dz) * v.ny + j + dy) * v.nx + i + dx
        den = f32(float(tq(vox[n])) - float(tq(vox[m])))
        s = min(max(div32(float(tq(vox[n])), den), 0.0), 1.0) if den != 0 else 0.0
        cn, cm = int(col[n]), int(col[m])
        if cn >> 24 and cm >> 24:
            out[-1] = 0xFF000000
            for sh in (0, 8, 16):
                out[-1] |= int(np.rint(np.float32(_lerp32(float((cn >> sh) & 0xFF), float((cm >> sh) & 0xFF), s)))) << sh
        elif cn >> 24:
            out[-1] = 0xFF000000 | cn
        elif cm >> 24:
            out[-1] = 0xFF000000 | cm
    return np.array(out, np.uint32)


@pytest.mark.parametrize("channels", [1, 4])
def test_restatement_equals_the_loops_and_the_plain_restatements(channels):
    v, s, poses, disp, mask, conf = small_scene()
    rng = np.random.default_rng(17)
    image = images_of(s, rng, channels)
    vox0, col0 = planted_start(v, rng)
    vox, col, stats = KR.integrate(vox0, col0, v, s, poses, disp, mask, conf, image, channels)
    want_vox, want_col = loop_integrate(vox0, col0, v, s, poses, disp, mask, conf, image, channels)
    assert np.array_equal(vox, want_vox) and np.array_equal(col, want_col)
    plain, updates = VR.integrate(vox0, v, s, poses, disp, mask, conf)
    assert np.array_equal(vox, plain) and stats["updates"] == updates > stats["colored"] > 20
    # the ray-cast: a view from the rotated camera, on the volume without masks so that rays find a surface
    vox, col, _ = KR.integrate(vox0, col0, v, s, poses, disp, None, None, image, channels)
    vw = scene_view(13, 9, frames=2, z_min=0.4, z_max=1.7, step=0.07)
    cams = np.stack([VR.pose(), VR.pose(np.eye(3), (0.05, -0.05, 0.1))])
    depth, normal, rgba, st = KR.raycast(vox, col, v, vw, cams)
    plain_d, plain_n, _ = RR.raycast(vox, v, vw, cams)
    same_maps("depth", depth, plain_d)
    same_maps("normal", normal, plain_n)
    assert np.array_equal(rgba, loop_raycast_colors(col, v, vw, cams, depth))
    assert st["trilinear"] + st["nearest"] + st["uncolored"] == st["hits"] > 10 and st["empty"] == depth.size - st["hits"]
    # the colours of the volume's own lists, and of ids that name nothing
    for kinds, recs in ((8, MR.vertices(vox, v, 1)), (4, VR.crossings(vox, v, 1))):
        ids = np.concatenate([recs["id"], invalid_ids(v, kinds)])
        assert np.array_equal(KR.colors(vox, col, v, ids, kinds), loop_colors(vox, col, v, ids, kinds)), kinds


# ---- the conditions the scenes meet --------------------------------------------------------------------------------------------

def test_the_coloured_scene_meets_every_condition_of_the_integration():
    v, s, poses, disp, image, vox0, col0 = colored_scene()
    vox, col, stats = KR.integrate(vox0, col0, v, s, poses, disp, None, None, image, 4)
    assert np.array_equal(vox, VR.integrate(vox0, v, s, poses, disp)[0])
    w, cw, cw0 = VR.unpack(vox)[1], KR.unpack(col)[3], KR.unpack(col0)[3]
    assert ((w > 0) & (cw == 0)).sum() > 100                     # sdf > trunc: distance, no colour
    assert stats["halves"] > 100 and stats["updates"] > stats["colored"] > 5000
    # the cap of eight bits: 254 -> 255 and 255 stays, in voxels that were painted
    changed = col != col0
    assert (changed & (cw0 == 254) & (cw == 255)).sum() > 20 and (changed & (cw0 == 255) & (cw == 255)).sum() > 20
    assert not (changed & (cw < cw0)).any()
    # the cap of max_weight, below 255: the planted 254 and 255 come down to it
    low = VR.spec(v.nx, v.ny, v.nz, v.voxel, v.origin, v.trunc, max_weight=2)
    col2 = KR.integrate(vox0, col0, low, s, poses, disp, None, None, image, 4)[1]
    cw2 = KR.unpack(col2)[3]
    assert cw2[col2 != col0].max() == 2 and ((col2 != col0) & (cw0 >= 254)).sum() > 40
    # one call over three frames is three calls of one frame
    a, b = vox0, col0
    for f in range(3):
        s1 = CR.spec(s.width, s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, baseline=s.baseline, frames=1)
        a, b, _ = KR.integrate(a, b, v, s1, poses[f:f + 1], disp[f:f + 1], None, None, image[f:f + 1], 4)
    assert np.array_equal(a, vox) and np.array_equal(b, col)
    # the top byte of a four-channel image is ignored, and grey is r = g = b
    assert np.array_equal(KR.integrate(vox0, col0, v, s, poses, disp, None, None, image & np.uint32(0xFFFFFF), 4)[1], col)
    grey = (image & np.uint32(0xFF)).astype(np.uint8)
    as_rgb = grey.astype(np.uint32) * np.uint32(0x010101)
    assert np.array_equal(KR.integrate(vox0, col0, v, s, poses, disp, None, None, grey, 1)[1],
                          KR.integrate(vox0, col0, v, s, poses, disp, None, None, as_rgb, 4)[1])


def test_the_slab_gives_the_raycast_all_four_pixel_classes():
    v, vox, col, slab = painted_scene()
    total = dict(trilinear=0, nearest=0, uncolored=0, empty=0)
    for w, h in ((24, 16), (70, 33), (33, 9)):
        st = KR.raycast(vox, slab, v, scene_view(w, h), VR.pose()[None])[3]
        for name in total:
            total[name] += st[name]
        assert st["trilinear"] > 0 and st["empty"] > 0, (w, h, st)
    assert min(total.values()) > 0, total
    rgba = KR.raycast(vox, col, v, scene_view(70, 33), VR.pose()[None])[2]
    assert set(np.unique(rgba >> 24).tolist()) == {0, 0xFF}


def test_the_lists_meet_all_four_colour_cases_and_every_invalid_edge():
    v, vox, col, slab = painted_scene()
    for kinds, recs in ((8, MR.vertices(vox, v, 1)), (4, VR.crossings(vox, v, 1))):
        assert set(KR.color_classes(vox, slab, v, recs["id"], kinds).tolist()) == {1, 2, 3}, kinds
        ids = invalid_ids(v, kinds)
        n, e = ids.astype(np.int64) // kinds, ids.astype(np.int64) % kinds
        classes = KR.color_classes(vox, col, v, ids, kinds)
        total = v.nx * v.ny * v.nz
        assert (n >= total).sum() >= 4 and np.all(classes[n >= total] == 0)                       # n out of range
        assert (e == kinds - 1).sum() > 30 and np.all(classes[e == kinds - 1] == 0)                # e == 7, or e == 3 with 4
        outside = (n < total) & (e == 0) & (n % v.nx == v.nx - 1)
        assert outside.sum() >= 2 and np.all(classes[outside] == 0)                              # the far voxel outside the grid
        top = (n < total) & (e == 2) & (n // (v.nx * v.ny) == v.nz - 1)
        assert top.sum() >= 2 and np.all(classes[top] == 0)
        assert (classes == 3).sum() > 20
        got = KR.colors(vox, col, v, ids, kinds)
        assert np.all(got[classes == 0] == 0) and np.all(got[classes == 3] >> 24 == 0xFF)


# ---- header, library, Python ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(S.library_path())
    return S.load_library()


ENTRIES = ("sgm_volume_integrate_color", "sgm_volume_raycast_color", "sgm_volume_colors")


def test_header_library_and_python_agree(lib):
    import soc_project_stereo_matching_amd as S
    from test_cabi import _declared_functions
    declared = _declared_functions()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name) and hasattr(lib, name.replace("sgm_", "sgmd_", 1)), name
        assert callable(getattr(S.SGMInstance, name[4:], None)), name
    with open(os.path.join(ROOT, "include", "sgm_mi355x.h")) as fh:
        text = fh.read()
    head = "colour in the TSDF volume: fused with the depth, ray-cast with it, given to the mesh"
    assert text.count(head) == 1 and text.index(head) > text.index("sgm_track_world_pose(const float")
    block = text.split(head)[1].split("bool sgm_volume_integrate_color(")[0]
    for line in ("(cw << 24) | (b << 16) | (g << 8) | r", "c = floor_div(2*(c*cw + p) + (cw + 1), 2*(cw + 1))", "cw = min(cw + 1, min(max_weight, 255))",
                 "sdf <= trunc", "h = g* - 0.5f, i0 = floorf(h)", "lerp(p, q, s) = p + s*(q - p)", "v = (unsigned)rintf(fminf(fmaxf(value, 0), 255))",
                 "0xFF000000 | b << 16 | g << 8 | r", "den = (float)tq[n] - (float)tq[m]", "s = den != 0 ? fminf(fmaxf((float)tq[n] / den, 0), 1) : 0",
                 "rintf(lerp(c_n, c_m, s))", "r < capacity and (d_count == NULL or r < d_count[0])", "capacity == 0 is a successful no-op"):
        assert line in block, line
    assert "Not part of it:" in block and "sgm_volume_spec;" not in block and "sgm_raycast_spec;" not in block
    # the earlier sections still list colour as not theirs, word for word
    assert "confidence-weighted updates, colour, voxel hashing" in text and "shading and colour, pose estimation" in text
    assert "vertex normals, colour, decimation" in text
    with open(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_host.c")) as fh:
        host_c = fh.read()
    for name in ENTRIES:
        assert "#pragma weak " + name.replace("sgm_", "sgmd_", 1) + "\n" in host_c, name


# ---- host logic on the stand-in device -----------------------------------------------------------------------------------------

def _sign(L):
    for name, (res, args) in {"sgm_volume_integrate_color": (_b, [_p] * 8 + [_i, _p, _p]), "sgm_volume_raycast_color": (_b, [_p] * 9),
                              "sgm_volume_colors": (_b, [_p] * 5 + [_z, _p, _i, _p]), "sgm_volume_integrate": (_b, [_p] * 8),
                              "sgm_volume_raycast": (_b, [_p] * 7), "sgm_volume_bytes": (_z, [_p]),
                              "stub_color_clear": (None, []), "stub_color_count": (_i, []), "stub_color_kind": (_i, [_i]),
                              "stub_color_ptr": (_p, [_i, _i]), "stub_color_int": (C.c_longlong, [_i, _i]),
                              "stub_color_volume": (C.POINTER(DeviceVolume), [_i]), "stub_color_src": (C.POINTER(DeviceSrc), [_i]),
                              "stub_color_view": (C.POINTER(DeviceView), [_i]), "stub_color_poses": (C.POINTER(C.c_float), [_i]),
                              "stub_color_fail_at": (None, [_i]), "stub_volume_clear": (None, []), "stub_volume_count": (_i, []),
                              "stub_raycast_clear": (None, []), "stub_raycast_count": (_i, [])}.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _sign(standin.build(tmp_path_factory.mktemp("colorstub"), extra_sources=[STUB_VOLUME, STUB_RAYCAST, STUB_COLOR], flags=("-ffp-contract=off",)))


@pytest.fixture(scope="module")
def host_without(tmp_path_factory):
    """the volume's and the ray-cast's launchers without the coloured ones"""
    return _sign(standin.build(tmp_path_factory.mktemp("colorstub_without"), extra_sources=[STUB_VOLUME, STUB_RAYCAST], flags=("-ffp-contract=off",)))


PAD = 8                                                           # words of 0xA5 on either side of an array


class Held:
    """a caller's "device" array on the stand-in: host words between two pads of 0xA5; data None: an output, 0xA5 inside too"""
    def __init__(self, words, data=None):
        self.n = words
        self.a = np.full(words + 2 * PAD, A5, np.uint32)
        if data is not None:
            self.a[PAD:PAD + words] = np.asarray(data).reshape(-1).view(np.uint32)
        self.before = self.a.copy()

    ptr = property(lambda self: self.a.ctypes.data + 4 * PAD)

    def untouched(self):
        return np.array_equal(self.a, self.before)

    def words(self):
        assert np.all(self.a[:PAD] == A5) and np.all(self.a[PAD + self.n:] == A5), "wrote outside the array"
        return self.a[PAD:PAD + self.n]


class Calls:
    """the buffers of the three calls on the coloured scene, and the calls themselves with any argument replaced"""
    def __init__(self, L, s):
        self.L, self.s = L, s
        self.v, self.src, self.poses, self.disp, self.image, vox0, col0 = colored_scene()
        self.vox0, self.col0 = vox0, col0
        self.n = vox0.size
        self.vox, self.col = Held(self.n, vox0), Held(self.n, col0)
        self.vw = scene_view(24, 16, frames=2)
        self.cams = moving_rig(2)
        self.px = 2 * 24 * 16
        self.depth, self.normal, self.rgba = Held(self.px), Held(3 * self.px), Held(self.px)
        self.recs = MR.vertices(KR.integrate(vox0, col0, self.v, self.src, self.poses, self.disp, None, None, self.image, 4)[0], self.v, 1)[:300]
        self.rec = Held(4 * len(self.recs), self.recs)
        self.count, self.out = Held(1, np.array([200], np.uint32)), Held(len(self.recs))
        self.all = (self.vox, self.col, self.depth, self.normal, self.rgba, self.rec, self.count, self.out)

    def untouched(self):
        return all(h.untouched() for h in self.all)

    def fuse(self, **kw):
        a = dict(s=self.s, spec=c_volume(self.v), src=c_source(self.src), poses=self.poses.ctypes.data, disp=self.disp.ctypes.data, mask=None,
                 conf=None, image=self.image.ctypes.data, channels=4, voxels=self.vox.ptr, colors=self.col.ptr)
        a.update(kw)
        ref = lambda t: None if t is None else C.byref(t)
        return self.L.sgm_volume_integrate_color(a["s"], ref(a["spec"]), ref(a["src"]), a["poses"], a["disp"], a["mask"], a["conf"], a["image"],
                                                 a["channels"], a["voxels"], a["colors"])

    def render(self, **kw):
        a = dict(s=self.s, vol=c_volume(self.v), view=c_view(self.vw), poses=self.cams.ctypes.data, voxels=self.vox.ptr, colors=self.col.ptr,
                 depth=self.depth.ptr, normal=self.normal.ptr, rgba=self.rgba.ptr)
        a.update(kw)
        ref = lambda t: None if t is None else C.byref(t)
        return self.L.sgm_volume_raycast_color(a["s"], ref(a["vol"]), ref(a["view"]), a["poses"], a["voxels"], a["colors"], a["depth"], a["normal"],
                                               a["rgba"])

    def paint(self, **kw):
        a = dict(s=self.s, spec=c_volume(self.v), voxels=self.vox.ptr, colors=self.col.ptr, records=self.rec.ptr, capacity=len(self.recs),
                 count=self.count.ptr, kinds=8, rgba=self.out.ptr)
        a.update(kw)
        return self.L.sgm_volume_colors(a["s"], None if a["spec"] is None else C.byref(a["spec"]), a["voxels"], a["colors"], a["records"],
                                        a["capacity"], a["count"], a["kinds"], a["rgba"])


def clear(L):
    L.stub_clear(); L.stub_volume_clear(); L.stub_raycast_clear(); L.stub_color_clear()


def test_the_validated_specs_the_poses_and_the_callers_pointers_arrive_and_the_stand_in_equals_the_restatement(host):
    L = host
    s = L.sgm_create(0)                                           # never initialised: explicit maps need no shape
    c = Calls(L, s)
    clear(L)
    assert c.fuse() and c.render() and c.paint() and c.paint(count=None, kinds=4)
    assert [L.stub_color_kind(k) for k in range(L.stub_color_count())] == [0, 1, 2, 2]
    assert standin.log(L) == []                                   # no scratch, no copy, no wait without a match in flight
    assert [L.stub_color_ptr(0, k) for k in range(7)] == [c.disp.ctypes.data, None, None, c.image.ctypes.data, c.vox.ptr, c.col.ptr, c.poses.ctypes.data]
    assert L.stub_color_int(0, 0) == 4
    assert bytes(L.stub_color_volume(0).contents) == bytes(c_volume(c.v)) and L.stub_color_src(0).contents.B == 3
    assert (L.stub_color_src(0).contents.W, L.stub_color_src(0).contents.H, L.stub_color_src(0).contents.fb) == (70, 33, 40.0)
    assert np.array_equal(np.ctypeslib.as_array(L.stub_color_poses(0), (36,)), c.poses.reshape(-1))
    assert [L.stub_color_ptr(1, k) for k in range(6)] == [c.vox.ptr, c.col.ptr, c.depth.ptr, c.normal.ptr, c.rgba.ptr, c.cams.ctypes.data]
    assert bytes(L.stub_color_volume(1).contents) == bytes(c_volume(c.v)) and bytes(L.stub_color_view(1).contents) == bytes(c_view(c.vw))
    assert np.array_equal(np.ctypeslib.as_array(L.stub_color_poses(1), (24,)), c.cams.reshape(-1))
    assert [L.stub_color_ptr(2, k) for k in range(5)] == [c.vox.ptr, c.col.ptr, c.rec.ptr, c.count.ptr, c.out.ptr]
    assert (L.stub_color_int(2, 0), L.stub_color_int(2, 1)) == (300, 8) and L.stub_color_ptr(3, 3) is None and L.stub_color_int(3, 1) == 4
    # what the stand-in computed: the restatement, word for word
    vox, col, _ = KR.integrate(c.vox0, c.col0, c.v, c.src, c.poses, c.disp, None, None, c.image, 4)
    assert np.array_equal(c.vox.words(), vox.reshape(-1)) and np.array_equal(c.col.words(), col.reshape(-1))
    depth, normal, rgba, stats = KR.raycast(vox, col, c.v, c.vw, c.cams)
    assert stats["trilinear"] > 100
    same_maps("depth", c.depth.words().view(np.float32), depth)
    same_maps("normal", c.normal.words().view(np.float32), normal)
    assert np.array_equal(c.rgba.words(), rgba.reshape(-1))
    assert np.array_equal(c.out.words(), KR.colors(vox, col, c.v, c.recs["id"], 4))      # the last call read the ids as n*4 + a
    out = Held(300)
    assert c.paint(rgba=out.ptr)
    assert np.array_equal(out.words()[:200], KR.colors(vox, col, c.v, c.recs["id"][:200], 8)) and np.all(out.words()[200:] == A5)
    # grey, the slab and the ids that name nothing
    c2 = Calls(L, s)
    grey = (c.image & np.uint32(0xFF)).astype(np.uint8)
    assert c2.fuse(image=grey.ctypes.data, channels=1)
    assert np.array_equal(c2.col.words(), KR.integrate(c.vox0, c.col0, c.v, c.src, c.poses, c.disp, None, None, grey, 1)[1].reshape(-1))
    slab = Held(c.n, slab_zeroed(c.v, col))
    assert c.render(colors=slab.ptr, normal=None)
    want = KR.raycast(vox, slab.words(), c.v, c.vw, c.cams)
    assert np.array_equal(c.rgba.words(), want[2].reshape(-1)) and min(want[3][k] for k in ("trilinear", "nearest", "uncolored", "empty")) > 0
    for kinds in (4, 8):
        ids = invalid_ids(c.v, kinds)
        recs = np.zeros(len(ids), MR.VERTEX)
        recs["id"] = ids
        rec, out = Held(4 * len(ids), recs), Held(len(ids))
        assert c.paint(records=rec.ptr, capacity=len(ids), count=None, kinds=kinds, rgba=out.ptr)
        assert np.array_equal(out.words(), KR.colors(vox, col, c.v, ids, kinds))
    L.sgm_destroy(s)


def refused(c, call, capfd, entry, **kw):
    """false, one line on stderr that names the entry point, nothing logged, nothing touched"""
    clear(c.L)
    capfd.readouterr()
    assert not call(**kw), kw
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("sgm_mi355x: %s: " % entry), (kw, err)
    assert c.L.stub_color_count() == 0 and c.L.stub_volume_count() == 0 and c.L.stub_raycast_count() == 0 and standin.log(c.L) == []
    assert c.untouched(), kw
    return err


def test_every_refusal_queues_nothing_and_prints_its_line(host, capfd):
    L = host
    s = L.sgm_create(0)
    c = Calls(L, s)
    x, k = c.vox.ptr, c.col.ptr
    vol_bytes, px_bytes = 4 * c.n, 4 * c.px
    src65 = c_source(CR.spec(70, 33, fx=40.0, fy=40.0, cx=34.5, cy=16.0, baseline=1.0, frames=65))
    bad_pose = c.poses.copy()
    bad_pose[1, 5] = NAN
    no_src = c_source(c.src)
    no_src.fx = 0.0
    f = lambda **kw: refused(c, c.fuse, capfd, "sgm_volume_integrate_color", **kw)
    for kw in (dict(s=None), dict(spec=None), dict(src=None), dict(poses=None), dict(voxels=None), dict(image=None), dict(colors=None)):
        assert "NULL argument" in f(**kw)
    for name, bad in sorted(VOLUME_REFUSALS.items()):
        assert "the volume spec is outside its ranges" in f(spec=c_volume(bad_volume(**bad))), name
    assert "the source spec is outside its ranges" in f(src=no_src) and "65 frames" in f(src=src65, poses=moving_rig(65).ctypes.data)
    assert "is not finite" in f(poses=bad_pose.ctypes.data)
    for ch in (0, 2, 3, 5, -1):
        assert "channels" in f(channels=ch)
    for kw in (dict(image=c.image.ctypes.data + 2), dict(image=c.image.ctypes.data + 1), dict(colors=k + 2), dict(colors=k + 1), dict(voxels=x + 2),
               dict(disp=c.disp.ctypes.data + 2)):
        assert "not aligned" in f(**kw)
    grey = np.zeros(c.disp.size + 1, np.uint8)
    clear(L)
    assert c.fuse(image=grey.ctypes.data + 1, channels=1) and L.stub_color_count() == 1         # a grey image needs no alignment
    c = Calls(L, s)
    x, k = c.vox.ptr, c.col.ptr
    f = lambda **kw: refused(c, c.fuse, capfd, "sgm_volume_integrate_color", **kw)
    img, dsp = c.image.ctypes.data, c.disp.ctypes.data
    for kw in (dict(colors=x), dict(colors=x + vol_bytes - 4), dict(colors=x - vol_bytes + 4), dict(colors=img), dict(colors=img + c.image.nbytes - 4),
               dict(colors=dsp), dict(colors=dsp - vol_bytes + 4), dict(mask=k), dict(conf=k + vol_bytes - 2), dict(voxels=img)):
        assert "overlap" in f(**kw) or "aliases" in f(**kw), kw
    assert "no map given" in f(disp=None)
    g = lambda **kw: refused(c, c.render, capfd, "sgm_volume_raycast_color", **kw)
    for kw in (dict(s=None), dict(vol=None), dict(view=None), dict(poses=None), dict(voxels=None), dict(colors=None), dict(depth=None), dict(rgba=None)):
        assert "NULL argument" in g(**kw)
    bad_view = c_view(c.vw)
    bad_view.step = 0.0
    assert "the view is outside its ranges" in g(view=bad_view) and "the volume spec is outside its ranges" in g(vol=c_volume(bad_volume(nx=0)))
    assert "is not finite" in g(poses=bad_pose.ctypes.data)
    d, n, r = c.depth.ptr, c.normal.ptr, c.rgba.ptr
    for kw in (dict(colors=k + 2), dict(rgba=r + 2), dict(rgba=r + 1), dict(depth=d + 2), dict(normal=n + 1), dict(voxels=x + 2)):
        assert "not aligned" in g(**kw)
    for kw in (dict(rgba=x), dict(rgba=x + vol_bytes - 4), dict(rgba=k), dict(rgba=k - px_bytes + 4), dict(rgba=d), dict(rgba=d + px_bytes - 4),
               dict(rgba=n), dict(rgba=n + 3 * px_bytes - 4), dict(depth=k), dict(normal=k + 16), dict(normal=d)):
        assert "overlaps" in g(**kw), kw
    h = lambda **kw: refused(c, c.paint, capfd, "sgm_volume_colors", **kw)
    for kw in (dict(s=None), dict(spec=None), dict(voxels=None), dict(colors=None), dict(records=None), dict(rgba=None)):
        assert "NULL argument" in h(**kw)
    for kinds in (0, 3, 5, 7, 16):
        assert "id_kinds" in h(kinds=kinds)
    assert "the volume spec is outside its ranges" in h(spec=c_volume(bad_volume(trunc=0.0)))
    assert "2^27" in h(spec=c_volume(VR.spec(1024, 1024, 129, 0.01, (0, 0, 0), 0.1)))
    q, t, o = c.rec.ptr, c.count.ptr, c.out.ptr
    for kw in (dict(records=q + 8), dict(records=q + 4), dict(voxels=x + 2), dict(colors=k + 1), dict(count=t + 2), dict(rgba=o + 2)):
        assert "not aligned" in h(**kw)
    for kw in (dict(rgba=x), dict(rgba=k + vol_bytes - 4), dict(rgba=q), dict(rgba=q + 16 * 300 - 4), dict(rgba=t), dict(count=o + 4 * 299),
               dict(rgba=x - 4 * 300 + 4)):
        assert "overlaps" in h(**kw), kw
    # allowed: capacity 0 with nothing to write; 2^27 voxels with mesh ids and more with point ids (the stand-in only logs them);
    # outputs that touch their neighbours
    clear(L)
    assert c.paint(records=None, capacity=0, count=None, rgba=None) and L.stub_color_count() == 0 and c.untouched()
    far = dict(voxels=1 << 44, colors=1 << 45, capacity=1)       # (never read: no host array of half a gigabyte is next to the outputs)
    assert c.paint(spec=c_volume(VR.spec(1024, 1024, 128, 0.01, (0, 0, 0), 0.1)), **far) and L.stub_color_count() == 1
    assert c.paint(spec=c_volume(VR.spec(1024, 1024, 129, 0.01, (0, 0, 0), 0.1)), kinds=4, **far) and L.stub_color_count() == 2
    L.sgm_destroy(s)


def test_host_without_the_launchers_links_refuses_and_keeps_the_plain_calls(host_without, capfd):
    L = host_without
    s = L.sgm_create(0)
    c = Calls(L, s)
    L.stub_clear(); L.stub_volume_clear(); L.stub_raycast_clear()
    for call, entry in ((c.fuse, "sgm_volume_integrate_color"), (c.render, "sgm_volume_raycast_color"), (c.paint, "sgm_volume_colors")):
        capfd.readouterr()
        assert not call()
        err = capfd.readouterr().err
        assert err.startswith("sgm_mi355x: %s: " % entry) and err.endswith("not part of this build\n") and err.count("\n") == 1, err
    assert standin.log(L) == [] and L.stub_volume_count() == 0 and L.stub_raycast_count() == 0 and c.untouched()
    assert L.sgm_volume_bytes(C.byref(c_volume(c.v))) == 4 * c.n
    assert L.sgm_volume_integrate(s, C.byref(c_volume(c.v)), C.byref(c_source(c.src)), c.poses.ctypes.data, c.disp.ctypes.data, None, None, c.vox.ptr)
    assert np.array_equal(c.vox.words(), VR.integrate(c.vox0, c.v, c.src, c.poses, c.disp)[0].reshape(-1))
    assert L.sgm_volume_raycast(s, C.byref(c_volume(c.v)), C.byref(c_view(c.vw)), c.cams.ctypes.data, c.vox.ptr, c.depth.ptr, c.normal.ptr)
    assert L.stub_volume_count() == 1 and L.stub_raycast_count() == 1
    L.sgm_destroy(s)


W, H = 48, 20


def test_plain_match_logs_what_it_logs_without_the_colour(host, host_without):
    """allocations and their sizes included: an instance that never calls the coloured entry points is the instance it was"""
    import soc_project_stereo_matching_amd as S
    left, right = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    out, conf = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint16)
    logs = []
    for L in (host, host_without):
        s = L.sgm_create(0)
        opt = S.default_option(16)
        L.stub_clear()
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        assert L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)                     # without Reset
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match_confidence(s, left.ctypes.data, right.ctypes.data, out.ctypes.data,
                                                                           conf.ctypes.data)
        assert L.sgm_set_overlap_post(s, 1)
        assert L.sgm_reset(s, W, H, C.byref(opt)) and L.sgm_match(s, left.ctypes.data, right.ctypes.data, out.ctypes.data)
        logs.append([(e.name, e.arg) for e in standin.log(L)])
        L.sgm_destroy(s)
    assert logs[0] == logs[1] and len(logs[0]) > 10
    host.stub_color_clear()
    assert host.stub_color_count() == 0


def test_a_refused_launch_or_wait_fails_the_call_and_the_calls_wait_for_a_match_in_flight(host):
    import soc_project_stereo_matching_amd as S
    L = host
    s = L.sgm_create(0)
    opt = S.default_option(16)
    c = Calls(L, s)
    for call in (c.fuse, c.render, c.paint):
        clear(L)
        L.stub_color_fail_at(0)
        assert not call() and L.stub_color_count() == 1 and c.untouched()
    # with the post pass on a stream of its own each call waits for the result of a match that is still in flight
    left = np.zeros((H, W), np.uint8)
    scratch = np.zeros((H, W), np.float32)
    assert L.sgm_set_overlap_post(s, 1) and L.sgm_reset(s, W, H, C.byref(opt))
    for call in (c.fuse, c.render, c.paint):
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        clear(L)
        assert call()
        assert "wait_event" in [e.name for e in standin.log(L)] and "alloc" not in [e.name for e in standin.log(L)]
        assert L.sgm_match_device(s, left.ctypes.data, left.ctypes.data, scratch.ctypes.data)
        clear(L)
        L.stub_fail_at(b"wait_event", 0)
        assert not call() and L.stub_color_count() == 0
        assert L.sgm_synchronize(s)
    L.sgm_destroy(s)


# ---- the driver on the stand-in ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("color_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"), STUB_VOLUME, STUB_RAYCAST, STUB_MESH,
                                        STUB_COLOR], libs=("-lz",))


def test_driver_usage_errors_are_told_apart(tmp_path):
    from test_driver_volume import EXE, PIN, VOLUME
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    pin = ",".join(PIN)
    base = [EXE, "a.png", "b.png", str(tmp_path / "o.png")]
    full = ["--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin]
    for extra, says in ((["--volume-color", "--pinhole", pin], "--volume-color needs --volume"),
                        (full + ["--volume-color", "--volume-image", "i.pgm"], "--volume-image OUT.pgm needs --volume-view"),
                        (full + ["--volume-view", "52,55,0.1", "--volume-image", "i.pgm"], "--volume-image OUT.pgm needs --volume-view")):
        out = subprocess.run(base + extra, capture_output=True, text=True)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    out = subprocess.run(base + full + ["--volume-color", "--volume-view", "52,55,0.1", "--volume-image", "i.pgm"], capture_output=True, text=True)
    assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


def test_driver_on_the_stand_in_writes_the_restatements_colours_and_without_the_flag_what_it_wrote(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75"""
    from test_driver_mesh import WIDE, read_mesh_ply, spec_of
    from test_driver_volume import PIN, write_pgm
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, mesh, plain_ply, plain_mesh, pgm, depth = (str(tmp_path / n) for n in ("d.f32", "v.ply", "m.ply", "pv.ply", "pm.ply", "i.pgm", "z.f32"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN), "--volume", WIDE]
    out = subprocess.run(base + ["--volume-ply", plain_ply, "--volume-mesh", plain_mesh], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    out = subprocess.run(base + ["--volume-ply", ply, "--volume-mesh", mesh, "--volume-color", "--volume-view", "40,60,1.5", "--volume-depth", depth,
                                 "--volume-image", pgm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    v = spec_of(WIDE)
    fx, fy, cx, cy, baseline, doffs = (float(x) for x in PIN)
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs)
    disp = np.fromfile(raw, np.float32).reshape(1, h, w)
    vox, col, stats = KR.integrate(VR.empty(v), KR.empty(v), v, s, VR.pose()[None], disp, None, None, img.reshape(1, h, w), 1)
    assert stats["colored"] > 1000
    vert, tri = MR.mesh(vox, v, 1)
    # without the flag: the file of the plain driver, byte for byte -- its header, the positions, the faces
    xyz, faces = read_mesh_ply(plain_mesh)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (len(vert), len(tri))).encode()
    face = np.zeros(len(tri), np.dtype([("n", "u1"), ("v", "<u4", (3,))]))
    face["n"], face["v"] = 3, tri["v"]
    positions = np.stack([vert["x"], vert["y"], vert["z"]], axis=1)
    assert open(plain_mesh, "rb").read() == head + positions.tobytes() + face.tobytes() and len(tri) > 500
    assert open(plain_ply, "rb").read() == open(ply, "rb").read()                             # the surface points' PLY does not change
    # with it: uchar red green blue behind every position, the restatement's
    body = open(mesh, "rb").read()
    head, body = body.split(b"end_header\n", 1)
    assert head.decode().splitlines()[2:] == [f"element vertex {len(vert)}", "property float x", "property float y", "property float z",
                                              "property uchar red", "property uchar green", "property uchar blue", f"element face {len(tri)}",
                                              "property list uchar uint vertex_indices"]
    rec = np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
    assert rec.itemsize == 15 and len(body) == 15 * len(vert) + 13 * len(tri)
    got = np.frombuffer(body[:15 * len(vert)], rec)
    want = KR.colors(vox, col, v, vert["id"], 8)
    assert got["xyz"].tobytes() == positions.tobytes() and body[15 * len(vert):] == face.tobytes()
    assert np.array_equal(got["rgb"], np.stack([want & 0xFF, (want >> 8) & 0xFF, (want >> 16) & 0xFF], axis=1).astype(np.uint8))
    assert (want >> 24 == 0xFF).sum() > 0.9 * len(vert) and len(np.unique(got["rgb"][:, 0])) > 50
    # the image: the red channel of the coloured ray-cast, 0 where the pixel is empty
    vw = RR.view(w, h, fx, fy, cx, cy, 40.0, 60.0, 1.5)
    want_d, _, rgba, st = KR.raycast(vox, col, v, vw, VR.pose()[None])
    assert st["trilinear"] > 500 and st["empty"] > 0
    same_maps("depth", np.fromfile(depth, np.float32), want_d)
    assert open(pgm, "rb").read() == b"P5\n%d %d\n255\n" % (w, h) + (rgba[0] & 0xFF).astype(np.uint8).tobytes()


# ---- sanitizers on a stand-alone program ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_color_host_is_asan_ubsan_clean(tmp_path):
    """tests/color_sanitize_driver.c: a program of its own, linked with the host, the stub device and the stand-in launchers."""
    exe = standin.build(tmp_path, sanitize=True, exe="color_sanitize_driver", flags=("-ffp-contract=off", "-static-libasan", "-static-libubsan"),
                        extra_sources=[os.path.join(ROOT, "tests", "color_sanitize_driver.c"), STUB_VOLUME, STUB_RAYCAST, STUB_MESH, STUB_COLOR])
    # the sanitizer runtimes are linked statically, so the program runs in the environment as it is: nothing is unset for it
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("color_sanitize_driver ok")


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------

def _kernel_name(mangled):
    m = re.match(r"_Z\d+(sgm_volume_[a-z]+_k)(?:I((?:L[ib]\d+E)+)E)?", mangled)
    if not m.group(2):
        return m.group(1)
    args = [n if kind == "i" else ("true" if n == "1" else "false") for kind, n in re.findall(r"L([ib])(\d+)E", m.group(2))]
    return "%s<%s>" % (m.group(1), ",".join(args))


def test_the_kernels_compile_without_scratch_and_the_plain_ones_as_the_parent_did(tmp_path):
    """the compile-time gate: no scratch and no spills in the new instantiations, and the plain ones with the figures the parent
    commit's source gave under the same command -- both tables are in profiles/volume_color_resources.txt"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", fh.read(), re.M | re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sgm_volume.hip"),
                          "-o", str(tmp_path / "sgm_volume.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for block in out.stderr.split("Function Name: ")[1:]:
        num = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))
        got[_kernel_name(block.split()[0])] = [num(r"TotalSGPRs"), num(r" VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"),
                                               num(r"Occupancy \[waves/SIMD\]"), num(r"SGPRs Spill"), num(r"VGPRs Spill")]
    new = ["sgm_volume_integrate_k<4,true>", "sgm_volume_integrate_k<1,true>", "sgm_volume_raycast_k<true,true>", "sgm_volume_raycast_k<false,true>",
           "sgm_volume_colors_k"]
    for name in new:
        sgpr, vgpr, scratch, lds, occ, s_spill, v_spill = got[name]
        assert scratch == 0 and s_spill == 0 and v_spill == 0 and lds == 0, (name, got[name])
    with open(os.path.join(ROOT, "profiles", "volume_color_resources.txt")) as fh:
        sections = fh.read().split("\n== ")
    tables = {}
    for sec in sections[1:]:
        rows = [ln.split() for ln in sec.splitlines() if ln.startswith("sgm_volume_")]
        # kernel | SGPR VGPR scratch LDS occ. spills
        tables[sec.split(" ==")[0]] = {r[0]: [int(x) for x in r[2:7]] + [int(x) for x in r[7].split("+")] for r in rows}
    assert tables["this commit"] == got
    plain = {"sgm_volume_integrate_k<4>": "sgm_volume_integrate_k<4,false>", "sgm_volume_integrate_k<1>": "sgm_volume_integrate_k<1,false>",
             "sgm_volume_raycast_k<true>": "sgm_volume_raycast_k<true,false>", "sgm_volume_raycast_k<false>": "sgm_volume_raycast_k<false,false>",
             "sgm_volume_count_k": "sgm_volume_count_k", "sgm_volume_scan_k": "sgm_volume_scan_k", "sgm_volume_emit_k": "sgm_volume_emit_k"}
    assert sorted(tables["the parent commit"]) == sorted(plain)
    for old, now in plain.items():
        assert tables["the parent commit"][old] == got[now], (old, tables["the parent commit"][old], got[now])
