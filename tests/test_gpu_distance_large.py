"""The distance kernels beyond one lap of their bounded grids, and at 2^30 voxels, where a voxel's byte offset leaves 32 bits -- needs
an MI355X.  The shapes are derived from the constants of csrc/sgm_distance.hip, read as tests/geometry_large.py reads the others: if
a constant changes, the shapes follow.  Tolerance 0, against tests/distance_ref.py; the outputs between margins of 0xA5 and pre-filled
with it, the volume checked as only read."""
import itertools

import numpy as np
import pytest

import distance_ref as DR
from geometry_large import constant
from test_distance_cpu import planted_words
from test_gpu_volume import c_volume
from test_gpu_volume_distance import check, device_field, spec_of

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

FAR = DR.FAR
c = lambda name: constant("sgm_distance.hip", name)
THREADS, X_WAVES, MAX_BLOCKS, ROW_WAVE, LINE_A = c("DIST_THREADS"), c("DIST_X_WAVES"), c("DIST_MAX_BLOCKS"), c("DIST_ROW_WAVE"), c("DIST_LINE_A")
ROW_LAP = MAX_BLOCKS * X_WAVES                                    # the rows (or, for short rows, the waves' sets of rows) one lap of the x pass takes


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: the distance field needs no shape
    yield i
    i.close()


def lap_shapes():
    """name -> (dims, what must exceed one lap, one lap): each the smallest of its row length that needs a second lap, partial"""
    out = {}
    layers = lambda rows, ny: -(-(rows + 1) // ny)
    nx = ROW_WAVE // 4                                            # four rows share a wave
    out["x pass, rows that share a wave"] = ((nx, 128, layers(4 * ROW_LAP, 128)), lambda d: -(-d[1] * d[2] // 4), ROW_LAP)
    nx = ROW_WAVE + 4
    out["x pass, a wave per row, four voxels per lane"] = ((nx, 64, layers(ROW_LAP, 64)), lambda d: d[1] * d[2], ROW_LAP)
    out["x pass, a wave per row, one voxel per lane"] = ((nx + 1, 64, layers(ROW_LAP, 64)), lambda d: d[1] * d[2], ROW_LAP)
    # lines of two voxels take the widest strip, 256 columns: four strips of a row of 1024 (or of 1023, loaded by element)
    per = MAX_BLOCKS // 4 + 1
    assert 2 <= LINE_A
    out["y pass, 16-byte loads"] = ((1024, 2, per), lambda d: 4 * d[2], MAX_BLOCKS)
    out["z pass, 16-byte loads"] = ((1024, per, 2), lambda d: 4 * d[1], MAX_BLOCKS)
    out["y pass, by element"] = ((1023, 2, per), lambda d: 4 * d[2], MAX_BLOCKS)
    out["z pass, by element"] = ((1023, per, 2), lambda d: 4 * d[1], MAX_BLOCKS)
    return out


LAPS = lap_shapes()


@pytest.mark.parametrize("name", list(LAPS))
def test_volumes_beyond_one_lap_of_the_grid(inst, name):
    dims, items, lap = LAPS[name]
    assert lap < items(dims) < 2 * lap, (name, items(dims), lap)
    words = planted_words(np.random.default_rng(len(name)), dims, 0.01, 1)
    got = check(inst, dims, words, 1, 3, 0, 0, name)
    assert (got[-1] != FAR).any() and (got[0] != FAR).any()      # the last layer, beyond the lap, holds more than FAR


@pytest.mark.parametrize("dims", [(256, 128, -(-(MAX_BLOCKS * THREADS * 4 + 1) // (256 * 128))), (129, 64, -(-(MAX_BLOCKS * THREADS + 1) // (129 * 64)))])
def test_fields_beyond_one_lap_of_the_grid(inst, dims):
    n, per = dims[0] * dims[1] * dims[2], 4 if dims[0] % 4 == 0 else 1
    assert MAX_BLOCKS * THREADS < n // per < 2 * MAX_BLOCKS * THREADS
    rng = np.random.default_rng(dims[0])
    o = rng.integers(0, 65026, (dims[2], dims[1], dims[0])).astype(np.uint16)
    i = rng.integers(0, 65026, (dims[2], dims[1], dims[0])).astype(np.uint16)
    o[rng.random(o.shape) < 0.3] = 0
    o[rng.random(o.shape) < 0.1], i[rng.random(o.shape) < 0.1] = FAR, FAR
    v = spec_of(dims, 0.05)
    assert device_field(inst, v, o, i, f"{dims} signed").tobytes() == DR.field(o, i, 0.05).tobytes()
    assert device_field(inst, v, o, None, f"{dims} unsigned").tobytes() == DR.field(o, None, 0.05).tobytes()


def test_the_largest_volume_2_to_the_30_voxels():
    """1024^3: the volume zeros (4 GiB) with a few sites planted near the eight corners and in the middle, the distances 2 GiB,
    r = 3, unknown = 0.  The boxes around the sites are read back and compared with the restatement of those boxes; every word
    outside them must be FAR -- counted on the device, and sampled slabs read back.  This is where a 32-bit byte offset goes wrong."""
    import torch
    import soc_project_stereo_matching_amd as S
    n, margin, r = 1 << 30, 64, 3
    need = 4 * n + 2 * n + 3 * n + (1 << 28)                       # the two arrays, the temporaries of the counting, and room
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the device reports {free >> 20} MiB free, the 1024^3 case needs {need >> 20} MiB")
    A5 = int(np.array([0xA5A5], np.uint16).view(np.int16)[0])
    site_word = int(np.array([0x00018000], np.uint32).view(np.int32)[0])
    clusters = []                                                 # (the box's lower corner, its edge, the sites)
    for corner in itertools.product((0, 1023), repeat=3):
        sign = [1 if x == 0 else -1 for x in corner]
        sites = [tuple(x + s * o for x, s, o in zip(corner, sign, off)) for off in ((0, 0, 0), (2, 1, 0), (0, 3, 3))]
        clusters.append((tuple(0 if x == 0 else 1016 for x in corner), 8, sites))
    clusters.append(((504, 504, 504), 16, [(512, 512, 512), (511, 513, 512), (509, 512, 515)]))
    src = torch.zeros(n, dtype=torch.int32, device="cuda")
    dst = torch.full((n + 2 * margin,), A5, dtype=torch.int16, device="cuda")
    planted = [p for _, _, sites in clusters for p in sites]
    at = torch.tensor([(p[2] * 1024 + p[1]) * 1024 + p[0] for p in planted], dtype=torch.int64, device="cuda")
    src[at] = site_word
    torch.cuda.synchronize()
    v = spec_of((1024, 1024, 1024))
    inst = S.SGMInstance(0)
    try:
        assert inst.volume_distance(c_volume(v), S.distance_spec(1, r, 0, 0), src.data_ptr(), dst.data_ptr() + 2 * margin) and inst.synchronize()
    finally:
        inst.close()
    assert bool((dst[:margin] == A5).all()) and bool((dst[n + margin:] == A5).all()), "wrote outside the distances"
    assert int(torch.count_nonzero(src)) == len(planted) and bool((src[at] == site_word).all()), "the volume is only read"
    cube = dst[margin:n + margin].view(1024, 1024, 1024)
    near = 0
    for lo, edge, sites in clusters:
        got = cube[lo[2]:lo[2] + edge, lo[1]:lo[1] + edge, lo[0]:lo[0] + edge].contiguous().cpu().numpy().view(np.uint16)
        site = np.zeros((edge, edge, edge), bool)
        for p in sites:
            site[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]] = True
        want = DR.transform(site, r)
        assert np.array_equal(got, want), (lo, np.argwhere(got != want)[:4].tolist())
        near += int((want != FAR).sum())
    assert near > 9 * 3 * 20
    for k in (0, 1, 9, 511, 517, 1014, 1023):                     # slabs: whole layers, whatever the boxes hold of them aside
        layer = cube[k].cpu().numpy().view(np.uint16)
        inside = sum(int((DR.transform(_sites_of(lo, edge, sites), r)[k - lo[2]] != FAR).sum()) for lo, edge, sites in clusters if lo[2] <= k < lo[2] + edge)
        assert int((layer != FAR).sum()) == inside, k
    assert int(torch.count_nonzero(cube != -1)) == near           # everything else is FAR


def _sites_of(lo, edge, sites):
    site = np.zeros((edge, edge, edge), bool)
    for p in sites:
        site[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]] = True
    return site
