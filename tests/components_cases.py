"""The cases of the components tests as builders: a plain helper module, no fixtures; shared by tests/test_zz_components_cpu.py (the
restatement against an independent flood fill, the stand-in) and tests/test_gpu_components.py (the library against the restatement).
The tile constants are read from the source, so the shapes follow them."""
import itertools

import numpy as np

import components_ref as CR
import volume_ref as VR
from geometry_large import constant

TX = constant("sgm_components.hip", "CC_TX")
TY = constant("sgm_components.hip", "CC_TY")
TZ = constant("sgm_components.hip", "CC_TZ")
MAX_BLOCKS = constant("sgm_components.hip", "CC_MAX_BLOCKS")
IN, OUT = 0x00018000, 0x00010005                                  # observed at weight 1: occupied, free
SMALL_DIMS = [(1, 1, 1), (TX - 1, 1, 1), (TX, 2, 2), (TX + 1, 3, 2), (TX + 1, TY + 1, TZ + 1)]
DENSITIES = (0.05, 0.30, 0.59, 0.95)
OPTIONS = list(itertools.product((6, 26), (0, 1), (0, 1)))        # connectivity, set, unknown


def spec_of(dims, voxel=0.0625, origin=(-1.125, -1.0, 0.5)):
    return VR.spec(*dims, voxel, origin, 0.25)


def random_words(rng, dims, density, min_weight=1):
    """about `density` of the voxels occupied (observed, tq < 0), a quarter of the others unobserved, the rest free, zero among them"""
    shape = (dims[2], dims[1], dims[0])
    occupied = rng.random(shape) < density
    observed = occupied | (rng.random(shape) < 0.75)
    w = np.where(observed, rng.integers(min_weight, 65536, shape), rng.integers(0, min_weight, shape)).astype(np.uint32)
    tq = np.where(occupied, rng.integers(-32768, 0, shape), rng.integers(0, 32768, shape)).astype(np.int16)
    tq = np.where(~occupied & (rng.random(shape) < 0.1), 0, tq).astype(np.int16)
    return (w << 16) | tq.view(np.uint16).astype(np.uint32)


def small_cases(dims):
    """(density, min_weight, words) of one of SMALL_DIMS"""
    n = SMALL_DIMS.index(dims)
    for m, density in enumerate(DENSITIES):
        min_weight = (1, 9)[(n + m) % 2]
        yield density, min_weight, random_words(np.random.default_rng(4300 + 10 * n + m), dims, density, min_weight)


def planted(dims, inside):
    """words of a volume whose occupied voxels are `inside` (bool [nz][ny][nx]), everything observed"""
    assert inside.shape == (dims[2], dims[1], dims[0])
    return np.where(inside, np.uint32(IN), np.uint32(OUT))


def checkerboard(dims):
    k, j, i = np.mgrid[0:dims[2], 0:dims[1], 0:dims[0]]
    return planted(dims, (i + j + k) % 2 == 0)


def u_across_a_face(axis):
    """two bars inside one tile that meet only in the neighbouring tile along `axis` (0: x, 1: y, 2: z): (dims, words)"""
    dims = [TX + 4, TY + 4, TZ + 4]
    inside = np.zeros((dims[2], dims[1], dims[0]), bool)
    t = (TX, TY, TZ)[axis]
    other = [a for a in range(3) if a != axis]
    for side in (1, 3):
        at = [0, 0, 0]
        at[other[0]], at[other[1]] = side, 1
        sl = [slice(at[2], at[2] + 1), slice(at[1], at[1] + 1), slice(at[0], at[0] + 1)]
        sl[2 - axis] = slice(1, t + 2)                            # from inside the first tile into the second
        inside[tuple(sl)] = True
    bridge = [slice(1, 2), slice(1, 2), slice(1, 2)]
    bridge[2 - axis] = slice(t + 1, t + 2)
    bridge[2 - other[0]] = slice(1, 4)
    inside[tuple(bridge)] = True
    return tuple(dims), planted(tuple(dims), inside)


def comb():
    """a spine in the second y-tile whose teeth all cross the face into the first, and teeth of a second comb between them that do
    not reach the spine; the two touch at one corner only, so they are two components at 6 and one at 26: (dims, words)"""
    dims = (2 * TX + 3, 2 * TY, 3)
    inside = np.zeros((dims[2], dims[1], dims[0]), bool)
    inside[1, TY + 2, :] = True                                   # the spine
    inside[1, 2:TY + 2, 0::4] = True                              # its teeth
    inside[1, 0:TY + 1, 2::4] = True                              # the other comb's teeth, joined along y = 0
    inside[1, 0, :] = True
    inside[1, 1, 1] = True                                        # diagonal to the first tooth at (0, 2)
    return dims, planted(dims, inside)


def serpentine(dims=None):
    """one path through every other voxel row of a volume three tiles long in each axis, rows joined at alternating ends: the
    deepest parent chains.  (dims, words, the number of its voxels)"""
    dims = dims or (3 * TX, 3 * TY, 3 * TZ)
    nx, ny, nz = dims
    inside = np.zeros((nz, ny, nx), bool)
    inside[0::2, 0::2, :] = True
    rows = [(y, z) for z in range(0, nz, 2) for y in (range(0, ny, 2) if z % 4 == 0 else reversed(range(0, ny, 2)))]
    for n, ((y0, z0), (y1, z1)) in enumerate(zip(rows, rows[1:])):
        x = nx - 1 if n % 2 == 0 else 0
        inside[(z0 + z1) // 2, (y0 + y1) // 2, x] = True
    return dims, planted(dims, inside), int(inside.sum())


def last_tile_only():
    """one component, all of it in the last tile: (dims, words)"""
    dims = (TX + 9, TY + 5, TZ + 3)
    inside = np.zeros((dims[2], dims[1], dims[0]), bool)
    inside[TZ + 1, TY + 1:TY + 4, TX + 2:TX + 7] = True
    return dims, planted(dims, inside)


def blobs():
    """components of 1, 2, 5, 5, 7 and 12 voxels apart from each other: (dims, words, sizes in order of first)"""
    dims = (TX + 6, 6, 5)
    inside = np.zeros((dims[2], dims[1], dims[0]), bool)
    inside[0, 0, 0] = True                                        # 1
    inside[0, 0, 3:5] = True                                      # 2
    inside[0, 2, 0:5] = True                                      # 5
    inside[0, 4, TX - 2:TX + 3] = True                            # 5, across the tile face
    inside[2, 0, 0:7] = True                                      # 7
    inside[2:4, 2:4, 0:3] = True                                  # 12
    return dims, planted(dims, inside), [1, 2, 5, 5, 7, 12]


def floor_and_boxes():
    """a floor slab of three voxel layers in y with two boxes standing on it: (v, words, the floor plane as (normal, anchor),
    clearance).  voxel 0.25 and origin (0, 0, 0): every centre and every s below is exact in float32.  The plane lies in the middle
    layer's centres; clearance one voxel: the layer above has s == clearance exactly and is excluded, the boxes begin above it."""
    dims = (TX + 8, 9, 7)
    v = VR.spec(*dims, 0.25, (0.0, 0.0, 0.0), 0.5)
    inside = np.zeros((dims[2], dims[1], dims[0]), bool)
    inside[:, 0:3, :] = True                                      # the floor: y layers 0, 1, 2
    inside[1:4, 3:7, 3:9] = True                                  # a box on it
    inside[2:6, 3:6, TX - 2:TX + 5] = True                        # another, across the tile face
    plane = (np.array([0.0, 1.0, 0.0], np.float32), np.array([0.0, 0.375, 0.0], np.float32))   # through the centres of layer 1
    return v, planted(dims, inside), plane, 0.25


def lattice(dims, period=5, size=3):
    """boxes of `size`^3 voxels every `period` voxels: (words, labels, objects) in closed form, without the restatement"""
    nx, ny, nz = dims
    i, j, k = np.arange(nx), np.arange(ny), np.arange(nz)
    inside = ((k % period < size)[:, None, None] & (j % period < size)[None, :, None] & (i % period < size)[None, None, :])
    first = (((k - k % period)[:, None, None] * ny + (j - j % period)[None, :, None]) * nx + (i - i % period)[None, None, :])
    labels = np.where(inside, first + 1, 0).astype(np.uint32)
    ci, cj, ck = (np.arange(0, n, period) for n in dims)
    ext = [np.minimum(c + size, n) - c for c, n in zip((ci, cj, ck), dims)]
    K, J, I = np.meshgrid(ck, cj, ci, indexing="ij")
    EK, EJ, EI = np.meshgrid(ext[2], ext[1], ext[0], indexing="ij")
    objects = np.zeros(K.size, CR.COMPONENT)
    objects["first"] = ((K * ny + J) * nx + I).reshape(-1)
    voxels = (EK * EJ * EI).reshape(-1)
    objects["voxels"] = voxels
    for a, (c, e) in enumerate(((I, EI), (J, EJ), (K, EK))):
        c, e = c.reshape(-1), e.reshape(-1)
        objects["lo"][:, a], objects["hi"][:, a] = c, c + e - 1
        objects["sum"][:, a] = (voxels // e) * (e * (2 * c + e - 1) // 2)
    return planted(dims, inside), labels, objects
