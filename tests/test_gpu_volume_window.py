"""A window of the TSDF volume on the device (extension; include/sgm_mi355x.h, the window section) against the numpy restatement
tests/window_ref.py -- needs an MI355X.  Tolerance 0 everywhere: words and bytes are compared.  Every array a call may write sits
between margins of 0xA5 and is pre-filled with it, so a word that was not written shows as one that was written wrongly; the
margins are checked afterwards and the inputs compared unchanged.  The scenes and their conditions are those of
tests/test_window_cpu.py, which holds them against the restatements alone."""
import numpy as np
import pytest

import mesh_ref as MR
import volume_ref as VR
import window_ref as WR
from test_gpu_raycast import Between
from test_gpu_volume import c_source, c_volume, same_volume, upload
from test_window_cpu import (COMMUTE_OFFSETS, TILING_SHIFTS, dyadic_scene, inside_of, parts_of, sphere_scene, triangle_floats, walk_reference,
                             walk_scene)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: a window needs no shape
    yield i
    i.close()


def spec_bytes(v):
    return bytes(c_volume(v))


def device_window(inst, src, offset, dims, d_vox, d_col, label, skew=(False, False)):
    """one call on device arrays (Between, d_col may be None): (the window's spec, its voxels, its colours or None) as Between"""
    import torch
    nbytes = 4 * dims[0] * dims[1] * dims[2]
    out_vox, out_col = Between(nbytes, skew=skew[0]), (Between(nbytes, skew=skew[1]) if d_col is not None else None)
    torch.cuda.synchronize()
    got = inst.volume_window(c_volume(src), offset, dims, d_vox.ptr, d_col.ptr if d_col is not None else None, out_vox.ptr,
                             out_col.ptr if d_col is not None else None)
    assert got is not None and inst.synchronize(), label
    assert bytes(got) == spec_bytes(WR.window_spec(src, offset, dims)), label
    return got, out_vox, out_col


def check(inst, src, offset, dims, vox, col, label, d_vox=None, d_col=None, skew=(False, False, False, False)):
    """one call against the restatement; vox, col: the host words (col None: without colours); d_vox, d_col: their device copies,
    made here unless given (then the caller checks them as only read)"""
    own = d_vox is None
    if own:
        d_vox, d_col = Between(vox.nbytes, vox, skew[0]), (Between(col.nbytes, col, skew[1]) if col is not None else None)
    _, out_vox, out_col = device_window(inst, src, offset, dims, d_vox, d_col, label, skew[2:])
    shape = (dims[2], dims[1], dims[0])
    same_volume(label + " voxels", out_vox.read(label + " voxels", np.uint32).reshape(shape), WR.window(vox, src, offset, dims))
    if col is not None:
        same_volume(label + " colours", out_col.read(label + " colours", np.uint32).reshape(shape), WR.window(col, src, offset, dims))
    if own:
        only_read(label, d_vox, vox, d_col, col)


def only_read(label, d_vox, vox, d_col, col):
    assert d_vox.read(label + " source").tobytes() == np.ascontiguousarray(vox).tobytes(), f"{label}: the source is only read"
    assert d_col is None or d_col.read(label + " source colours").tobytes() == np.ascontiguousarray(col).tobytes(), f"{label}: the colours are only read"


def random_words(rng, dims):
    """any words, 0 and 0xFFFFFFFF among them"""
    words = rng.integers(0, 1 << 32, (dims[2], dims[1], dims[0]), dtype=np.uint64).astype(np.uint32)
    words.reshape(-1)[::7] = 0xFFFFFFFF
    words.reshape(-1)[3::11] = 0
    return words


SMALL = [(5, 3, 2), (8, 4, 3), (13, 5, 3)]


# ---- 1. every edge of the copy -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", SMALL)
def test_every_edge_of_the_copy(inst, a):
    rng = np.random.default_rng(100 + a[0])
    src = VR.spec(*a, 0.0625, (-1.125, -1.0, 0.5), 0.25, max_weight=9)
    vox, col = random_words(rng, a), random_words(rng, a)
    d_vox, d_col = Between(vox.nbytes, vox), Between(col.nbytes, col)
    calls = 0
    for b in SMALL:
        ys, zs = (-b[1], 0, 1), (-1, 0, a[2])                      # the first y and the last z leave the source entirely
        for ox in range(-a[0] - 1, b[0] + 2):
            for oy in ys:
                for oz in zs:
                    color = calls % 2 == 0
                    check(inst, src, (ox, oy, oz), b, vox, col if color else None, f"{a} -> {b} at {(ox, oy, oz)} colours={color}", d_vox,
                          d_col if color else None)
                    calls += 1
    assert calls > 400
    only_read(str(a), d_vox, vox, d_col, col)


# ---- 2. alignment --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_nx", [36, 37])
def test_every_array_in_turn_one_word_off_a_16_byte_boundary(inst, src_nx):
    """dims (36, 33, 20): four voxels per lane and 16-byte loads where everything allows it; an array 4 bytes off, an x offset that
    is no multiple of 4 or a source row of 37 words takes the loads, or the stores as well, element by element"""
    rng = np.random.default_rng(200 + src_nx)
    a, b = (src_nx, 33, 20), (36, 33, 20)
    src = VR.spec(*a, 0.0625, (-1.125, -1.0, 0.5), 0.25)
    vox, col = random_words(rng, a), random_words(rng, a)
    none = (False, False, False, False)
    skews = [none] + [tuple(k == which for k in range(4)) for which in range(4)] + [(True, True, True, True)]
    for skew in skews:
        for ox in range(8):
            check(inst, src, (ox, -1, 2), b, vox, col, f"source nx={src_nx} skew={skew} ox={ox}", skew=skew)
    check(inst, src, (-4, 0, 0), b, vox, None, f"source nx={src_nx} without colours", skew=none)
    check(inst, src, (-3, 0, 0), b, vox, None, f"source nx={src_nx} without colours, skewed", skew=(True, False, True, False))


# ---- 3. algebra ----------------------------------------------------------------------------------------------------------------

def test_a_copy_the_composition_of_two_windows_and_two_runs(inst):
    rng = np.random.default_rng(300)
    a = (36, 33, 20)
    src = VR.spec(*a, 0.0625, (-1.125, -1.0, 0.5), 0.25)
    vox, col = random_words(rng, a), random_words(rng, a)
    d_vox, d_col = Between(vox.nbytes, vox), Between(col.nbytes, col)
    spec, out_vox, out_col = device_window(inst, src, (0, 0, 0), a, d_vox, d_col, "copy")
    assert bytes(spec) == spec_bytes(src)
    assert out_vox.read("copy").tobytes() == vox.tobytes() and out_col.read("copy colours").tobytes() == col.tobytes()
    # window(window(V, p, big), q) == window(V, p + q) where the intermediate loses nothing: it holds the whole source
    p, big = (-9, -6, -3), (60, 50, 30)
    for q, dims in (((13, 2, 5), a), ((1, 17, 0), (21, 9, 40)), ((9, 6, 3), a), ((30, -40, 2), (8, 8, 8))):
        mid_spec, mid_vox, mid_col = device_window(inst, src, p, big, d_vox, d_col, f"p={p}")
        mid = WR.window_spec(src, p, big)
        two = device_window(inst, mid, q, dims, mid_vox, mid_col, f"q={q}")
        sum_pq = tuple(x + y for x, y in zip(p, q))
        one = device_window(inst, src, sum_pq, dims, d_vox, d_col, f"p+q={sum_pq}")
        assert bytes(two[0]) == bytes(one[0]), q
        assert two[1].read("two").tobytes() == one[1].read("one").tobytes() == WR.window(vox, src, sum_pq, dims).tobytes(), q
        assert two[2].read("two colours").tobytes() == one[2].read("one colours").tobytes(), q
        assert mid_vox.read("mid").tobytes() == WR.window(vox, src, p, big).tobytes()
    runs = [device_window(inst, src, (5, -2, 1), a, d_vox, d_col, "run") for _ in range(2)]
    assert runs[0][1].read("run").tobytes() == runs[1][1].read("run").tobytes() and runs[0][2].read("run").tobytes() == runs[1][2].read("run").tobytes()
    only_read("algebra", d_vox, vox, d_col, col)


# ---- 4. windowing commutes with integration on a dyadic lattice ----------------------------------------------------------------

def device_integrate(inst, spec, s, poses, maps, d_vox, label):
    """spec: the ctypes spec, as volume_window hands it out"""
    assert inst.volume_integrate(spec, c_source(s), poses, maps.data_ptr(), None, None, d_vox.ptr) and inst.synchronize(), label


@pytest.mark.parametrize("offset", COMMUTE_OFFSETS)
def test_windowing_commutes_with_integration_on_a_dyadic_lattice(inst, offset):
    import torch
    v, s, poses, disp, vox0 = dyadic_scene()
    dims, shape = (v.nx, v.ny, v.nz), (v.nz, v.ny, v.nx)
    maps = upload(disp)
    torch.cuda.synchronize()
    # integrate, then window
    d_a = Between(vox0.nbytes, vox0)
    device_integrate(inst, c_volume(v), s, poses, maps, d_a, "integrate first")
    fused = d_a.read("fused", np.uint32).reshape(shape).copy()
    same_volume("the integration", fused, VR.integrate(vox0, v, s, poses, disp)[0])
    _, d_first, _ = device_window(inst, v, offset, dims, d_a, None, "then window")
    first = d_first.read("first", np.uint32).reshape(shape)
    # window, then integrate under the window's spec
    d_b = Between(vox0.nbytes, vox0)
    w, d_second, _ = device_window(inst, v, offset, dims, d_b, None, "window first")
    device_integrate(inst, w, s, poses, maps, d_second, "then integrate")
    second = d_second.read("second", np.uint32).reshape(shape)
    inside = inside_of(v, offset, dims)
    assert np.array_equal(first[inside], second[inside]), f"{offset}: {(first[inside] != second[inside]).sum()} words inside differ"
    assert np.all(first[~inside] == 0) and (second[~inside] != 0).sum() >= 10, (offset, (second[~inside] != 0).sum())
    same_volume("window then integrate", second, VR.integrate(WR.window(vox0, v, offset, dims), WR.window_spec(v, offset, dims), s, poses, disp)[0])
    assert maps.cpu().numpy().tobytes() == np.ascontiguousarray(disp).tobytes()


# ---- 5. what leaves plus what stays is the whole mesh --------------------------------------------------------------------------

def device_mesh(inst, spec, d_vox, d_col, label):
    """(vertices, triangles, rgba or None) of the volume at d_vox (Between) under spec: a counts-only call, then the lists"""
    import torch
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert inst.volume_mesh(spec, d_vox.ptr, 1, None, 0, None, 0, counts.data_ptr()) and inst.synchronize(), label
    nv, nt = (int(x) for x in counts.cpu().numpy().view(np.uint32))
    vert, tri, rgba = Between(16 * max(nv, 1)), Between(16 * max(nt, 1)), Between(4 * max(nv, 1))
    torch.cuda.synchronize()
    assert inst.volume_mesh(spec, d_vox.ptr, 1, vert.ptr if nv else None, nv, tri.ptr if nt else None, nt, counts.data_ptr()), label
    if d_col is not None and nv:
        assert inst.volume_colors(spec, d_vox.ptr, d_col.ptr, vert.ptr, nv, counts.data_ptr(), 8, rgba.ptr), label
    assert inst.synchronize(), label
    return (vert.read(label + " vertices")[:16 * nv].view(MR.VERTEX), tri.read(label + " triangles")[:16 * nt].view(MR.TRIANGLE),
            rgba.read(label + " rgba", np.uint32)[:nv] if d_col is not None else None)


@pytest.mark.parametrize("shift", TILING_SHIFTS)
def test_what_leaves_plus_what_stays_is_the_whole_mesh(inst, shift):
    v, words = sphere_scene()
    d_vox = Between(words.nbytes, words)
    vert, tri, _ = device_mesh(inst, c_volume(v), d_vox, None, "whole")
    whole = triangle_floats(vert, tri)
    assert whole.tobytes() == triangle_floats(*MR.mesh(words, v, 1)).tobytes() and len(whole) > 1000
    rows = []
    for lo, n in parts_of(v, shift):
        spec, d_part, _ = device_window(inst, v, lo, n, d_vox, None, f"{shift}: box {lo} {n}")
        part = triangle_floats(*device_mesh(inst, spec, d_part, None, f"{shift}: box {lo} {n}")[:2])
        assert len(part) >= 100, (shift, lo, n, len(part))
        rows.append(part)
    rows = np.concatenate(rows)
    assert rows[np.lexsort(rows.T[::-1])].tobytes() == whole.tobytes(), shift
    assert d_vox.read("whole").tobytes() == words.tobytes()


# ---- 6. a rig that walks out of its first box ----------------------------------------------------------------------------------

def test_a_rig_that_walks_out_of_its_first_box(inst):
    """the documented loop on the device -- follow, window and mesh what leaves, shift into the other pair of arrays, integrate the
    frame with its colours -- against the same loop in numpy: after every step the words, the colours and every streamed mesh"""
    import torch
    import soc_project_stereo_matching_amd as S
    v, s1, poses, disp, image = walk_scene()
    maps, images = upload(disp), upload(image)
    torch.cuda.synchronize()
    px = s1.width * s1.height

    def window(spec, offset, dims, vox, col):
        got, out_vox, out_col = device_window(inst, spec, offset, dims, vox, col, f"window {offset} {dims}")
        return WR.window_spec(spec, offset, dims), out_vox, out_col

    def integrate(spec, f, vox, col):
        assert inst.volume_integrate_color(c_volume(spec), c_source(s1), poses[f:f + 1], maps.data_ptr() + 4 * f * px, None, None,
                                           images.data_ptr() + 4 * f * px, 4, vox.ptr, col.ptr) and inst.synchronize(), f
        return vox, col

    def mesh(spec, vox, col):
        return device_mesh(inst, c_volume(spec), vox, col, "streamed")

    # the loop of test_window_cpu.walk on device arrays, from an empty volume, with the library's own follow and leaving
    n = v.nx * v.ny * v.nz
    start = np.zeros(n, np.uint32)
    state = {"vox": Between(4 * n, start), "col": Between(4 * n, start)}
    want = walk_reference()
    spec = v
    for f, (shift, w_spec, w_vox, w_col, w_streamed) in enumerate(want):
        assert S.volume_follow(c_volume(spec), poses[f], 1.125, 4, 2) == shift, f
        boxes = S.volume_leaving(c_volume(spec), shift)
        assert boxes == [(lo, n_) for lo, n_, *_ in w_streamed], f
        for (lo, n_), (_, _, w_vert, w_tri, w_rgba) in zip(boxes, w_streamed):
            part = window(spec, lo, n_, state["vox"], state["col"])
            vert, tri, rgba = mesh(*part)
            assert vert.tobytes() == w_vert.tobytes() and tri.tobytes() == w_tri.tobytes() and rgba.tobytes() == w_rgba.tobytes(), (f, lo, n_)
        if any(shift):
            spec, state["vox"], state["col"] = window(spec, shift, (spec.nx, spec.ny, spec.nz), state["vox"], state["col"])
        integrate(spec, f, state["vox"], state["col"])
        assert spec_bytes(spec) == spec_bytes(w_spec), f
        shape = (spec.nz, spec.ny, spec.nx)
        same_volume(f"step {f} voxels", state["vox"].read(f"step {f} voxels", np.uint32).reshape(shape), w_vox)
        same_volume(f"step {f} colours", state["col"].read(f"step {f} colours", np.uint32).reshape(shape), w_col)
    assert sum(any(st[0]) for st in want) >= 2 and max(len(st_tri) for st in want for *_, st_tri, _ in st[4]) >= 50
    assert maps.cpu().numpy().tobytes() == np.ascontiguousarray(disp).tobytes() and images.cpu().numpy().tobytes() == np.ascontiguousarray(image).tobytes()
