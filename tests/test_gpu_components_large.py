"""Connected components on the device beyond one lap of every kernel's grid and beyond one chunk of the compaction's scan (extension;
include/sgm_mi355x.h, the components section) -- needs an MI355X.  The volume is a lattice of small boxes (tests/components_cases.py,
lattice), so the labels and every record are known in closed form and the restatement never runs on it; the shape is derived from the
constants of the sources.  And one long thin volume at nx = 1024.  Tolerance 0."""
import numpy as np
import pytest

import components_cases as CC
import components_ref as CR
from geometry_large import CHUNK, TILE_MAX
from test_gpu_components import REC, check, device_components, inst  # noqa: F401  (inst: the module's instance fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

SY = CC.constant("sgm_components.hip", "CC_SY")
SZ = CC.constant("sgm_components.hip", "CC_SZ")
THREADS = CC.constant("sgm_components.hip", "CC_THREADS")


def big_dims():
    """the smallest number of layers of 256 x 192 voxels that is more than one lap of the tile kernel (the longest lap of all: the
    statistics tile and the striding launches take fewer voxels a block) and more than one chunk of the scan's tiles"""
    nx, ny = 4 * CC.TX, 24 * CC.TY
    tiles = lambda nz: (nx // CC.TX) * (ny // CC.TY) * -(-nz // CC.TZ)
    nz = 1
    while tiles(nz) <= CC.MAX_BLOCKS or nx * ny * nz <= CHUNK * TILE_MAX:
        nz += 1
    return nx, ny, nz + 3                                         # (not a multiple of the tile: a partial last layer of tiles)


def test_the_shape_is_beyond_one_lap_of_every_grid_and_one_chunk_of_the_scan():
    nx, ny, nz = big_dims()
    n = nx * ny * nz
    assert (nx // CC.TX) * (ny // CC.TY) * -(-nz // CC.TZ) > CC.MAX_BLOCKS                 # the tile kernel
    assert (nx // CC.TX) * (ny // SY) * -(-nz // SZ) > CC.MAX_BLOCKS                       # the statistics
    assert n > CC.MAX_BLOCKS * THREADS and -(-n // TILE_MAX) > CHUNK                       # the striding launches; the scan
    assert n * 4 < 1 << 27                                                                 # (and still a small array)


def test_a_lattice_of_boxes_beyond_one_lap_and_one_scan_chunk(inst):
    dims = big_dims()
    words, labels, objects = CC.lattice(dims)
    C = len(objects)
    assert C > CHUNK                                              # more records than tiles in a chunk: bases carry
    for connectivity in (6, 26):
        got_labels, raw, counts = device_components(inst, CC.spec_of(dims), words, f"lattice {dims} conn {connectivity}", connectivity=connectivity,
                                                    capacity=C + 1)
        assert tuple(counts) == (C, C)
        assert np.array_equal(got_labels, labels)
        assert raw[:REC * C].tobytes() == objects.tobytes() and np.all(raw[REC * C:] == 0xA5)
    # the filter: only whole boxes stay, the cut ones at the far faces go; the list is cut by its capacity
    whole = objects["voxels"] == 27
    assert 0 < whole.sum() < C
    got_labels, raw, counts = device_components(inst, CC.spec_of(dims), words, "whole boxes only", min_voxels=27, capacity=1000)
    assert tuple(counts) == (int(whole.sum()), C)
    keep = np.zeros(labels.max() + 1, bool)
    keep[objects["first"][whole] + 1] = True
    assert np.array_equal(got_labels, np.where(keep[labels], labels, 0))
    assert raw[:REC * 1000].tobytes() == objects[whole][:1000].tobytes()


def test_a_long_thin_volume_of_1024_voxel_rows(inst):
    dims = (1024, 3, 2)
    v = CC.spec_of(dims)
    for density in (0.3, 0.95):
        words = CC.random_words(np.random.default_rng(int(100 * density)), dims, density)
        for connectivity, set_, unknown in ((6, 0, 0), (26, 0, 1), (6, 1, 0)):
            check(inst, v, words, f"{dims} density {density} conn {connectivity} set {set_} unknown {unknown}", connectivity=connectivity,
                  set=set_, unknown=unknown)
    full = np.full((2, 3, 1024), CC.IN, np.uint32)
    (labels, raw, counts), _ = check(inst, v, full, "one row-spanning component")
    assert tuple(counts) == (1, 1) and tuple(raw[:REC].view(CR.COMPONENT)[0]["hi"]) == (1023, 2, 1)
