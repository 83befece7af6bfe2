"""Batches past 8 frames, as lists of cases: sgm_set_batch admits 1 to 1024 frames per call (csrc/sgm_host.c), and several launch
decisions depend on the batch B alone.  A plain helper module, no fixtures; shared by tests/test_batch_cpu.py (the oracle alone and
the C host on the stand-in device) and tests/test_gpu_batch_large.py (the library against the oracle, frame by frame).  Every
branch named here is established by ARITHMETIC from the launcher as it stands, restated beside the list that uses it; DESIGN.md
section 2 has the batch row of the table of limits, NOTES.md the table of B values.

Frame content: oracle.synth_pair with a different seed per frame (frame_seed), so that a kernel that reads another frame's cells
never goes unseen."""
import functools

import numpy as np

import instance_steps as IR

BATCH_MAX = 1024                                   # sgm_set_batch: 1 .. 1024
OPTION = dict(min_speckle_area=10)                 # the small frames keep more than the default area of 50 leaves them


def frame_seed(seed, frame):
    return seed + 7 * frame


def frames(oracle, w, h, d, batch, seed):
    """([(left, right)] * batch, L [B][H][W], R [B][H][W]): another seed per frame"""
    pairs = [oracle.synth_pair(w, h, d, frame_seed(seed, j)) for j in range(batch)]
    return pairs, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def option(d, dmin=0, **kw):
    from oracle.pyoracle import default_option
    return default_option(d + dmin, dmin, **dict(OPTION, **kw))


def padded_stride(D):
    """pick_dpl of csrc/sgm_host.c: 16 lanes of 2, 4, 8, 12, 16 or 32 disparities"""
    for dp in (32, 64, 128, 192, 256, 512):
        if D <= dp:
            return dp
    raise ValueError(D)


# ------------------------------------------------------------------------------------ a. every stage at the untested numberings
# sgm_aggregate.hip: strips = 8 / B for B in {1, 2, 4} (B < 8 and 8 % B == 0), the plain numbering frame = blockIdx.x % B for
# every other B; with the non-negative-P1 kernels the anomalous lines are the first 4 * B blocks, block = frame + B * (dir - 4).
def aggregation_numbering(batch):
    return "strips" if batch < 8 and 8 % batch == 0 and batch > 1 else "plain"      # (one frame: strips = 1, the plain formula at B = 1)


STAGE_BATCHES = {5: "plain numbering, odd, below 8", 6: "plain numbering, even, shares a factor with 8",
                 7: "plain numbering, the last B below one frame per XCD", 9: "plain numbering, the first B past one frame per XCD",
                 16: "plain numbering, two frames per XCD", 17: "plain numbering, odd, past 16"}
# (w, h, d): wide, W > H; tall, W < H: the diagonal planes are cleared per match (ghost_zero is false)
STAGE_SHAPES = [(64, 16, 16), (30, 70, 8)]
STAGE_SEED = 0xBA7C5000


# ------------------------------------------------------------------------------------------ b. segment choice by batch alone
SUMLR_MAX_EXTRA = 8                                # csrc/sgm_sum_wta.hip
LDS_BYTES, CUS, WAVES_PER_CU = 160 << 10, 256, 32


def sum_slots(dp, tight=True):
    """the residency estimate of sgmd_sum_wta_lr_conf: 256 CUs x what the ring (LDS) and the wave count of a workgroup allow"""
    threads = (1024 if tight else 512) if dp == 192 else (512 if tight else 256) if dp == 256 else 256
    ring_cols = dp + (1 if dp in (192, 256) and tight else 2) * (threads // 16) + dp // 16
    lds = ring_cols * (dp + 2) * 2 + SUMLR_MAX_EXTRA * dp + 64
    return CUS * min(LDS_BYTES // lds, WAVES_PER_CU // (threads // 64))


def sum_segments(w, h, d, batch):
    """(segments per row, True where the fallback decided): sgmd_sum_wta_lr_conf without SGM_SUM_SEGMENTS, without a kept or
    accumulated S"""
    dp = padded_stride(d)
    rows = h * batch
    segs = min((1024 + rows - 1) // rows, 4)
    while segs > 1 and w // segs < 2 * dp:
        segs -= 1
    segs = max(segs, 1)
    for sg in (4, 3, 2, 1):
        if rows * sg <= sum_slots(dp) and (sg == 1 or w // sg >= 2 * dp):
            return sg, False
    return segs, True


# 256 x 16, D = 32: Dp = 32, 256 threads, ring_cols = 32 + 2 * 16 + 2 = 66, lds = 66 * 34 * 2 + 8 * 32 + 64 = 4808 bytes, by_lds = 34,
# by_waves = 32 / 4 = 8: slots = 256 * 8 = 2048.  rows = 16 B; every count down to 2 keeps W / sg >= 2 Dp = 64 (256 / 4 = 64).
#   4 segments while 64 B <= 2048: B <= 32        3 while 48 B <= 2048: B <= 42        2 while 32 B <= 2048: B <= 64
#   1 while 16 B <= 2048: B <= 128                above: no count fits, the first formula decides: ceil(1024 / (16 B)) = 1
# test_batch_cpu.py asserts these from sum_segments.
SEGMENT_SHAPE = (256, 16, 32)
SEGMENT_BATCHES = {32: (4, False), 33: (3, False), 42: (3, False), 43: (2, False), 64: (2, False), 65: (1, False),
                   128: (1, False), 129: (1, True)}
SEGMENT_SEED = 0x5E65000


# ---------------------------------------------------------------------------------------------------- c. the admitted maximum
MAX_SHAPE = (24, 16, 8)                            # the suite's smallest shape
MAX_SEED = 0x3A8000
# queue_outputs of csrc/sgm_host.c: a staged (pageable) first result of RESULT_CHUNK_MIN bytes or more comes back in 2 pieces
# below RESULT_CHUNK_SPLIT and in RESULT_CHUNKS pieces from there on
RESULT_CHUNK_MIN, RESULT_CHUNK_SPLIT, RESULT_CHUNKS = 256 << 10, 4 << 20, 4
# 1024 maps of 24 x 16: 1.5 MiB, two pieces.  64 maps of 260 x 64: 4.06 MiB, RESULT_CHUNKS pieces; 260 is no multiple of 16
CHUNK_CASE = (260, 64, 16, 64)                     # (w, h, d, batch)
CHUNK_SEED = 0xC4A000


def result_chunks(w, h, batch):
    n = 4 * w * h * batch
    return 1 if n < RESULT_CHUNK_MIN else 2 if n < RESULT_CHUNK_SPLIT else RESULT_CHUNKS


# ------------------------------------------------------------------------------------------------- d. variants in a batch
VARIANT_BATCHES = (5, 9)
_V = (64, 16, 16)


def _rect_maps(w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x + 3, y - 2, x - 1, y


# name -> keyword arguments of instance_steps.step at _V (the windows need frames taller than they are: 64 x 16 admits 7 x 7)
VARIANTS = {
    "paths4": dict(paths4=True),
    "negative_p1": dict(pen=(-5, 150)),          # the generic step: back to 16 lanes per pixel, HL = 0
    "centre7x7": dict(window=(7, 7)),              # u64 words, the volume-fed aggregation: 16 lanes
    "symmetric7x7": dict(kind=IR.SYMMETRIC, window=(7, 7)),
    "right_view": dict(view=True),
    "confidence": dict(entry="confidence"),
    "fill": dict(fill=True),
    "refine": dict(refine=True),                   # (the instance's defaults: 2 iterations, asserted by the test)
    "bits12": dict(bits=12),
    "rectify": dict(rect="maps"),                  # one set of maps for all frames
    "q14": dict(q14=True),                         # a second match without Reset: the accumulate path, one segment
}
VARIANT_SEED = 0x7A21000


def variant_step(name, batch):
    kw = dict(VARIANTS[name])
    w, h, d = _V
    if kw.get("rect"):
        kw["rect"] = _rect_maps(w, h)
    return IR.step(w, h, d, batch=batch, **kw)


def variant_frames(oracle, st, seed):
    """as frames(); more than 8 bits per sample: the u8 pair shifted up with random low bits (tests/scaled_cases.py, scene)"""
    pairs, L, R = frames(oracle, st["w"], st["h"], st["d"], st["batch"], seed)
    if st["bits"] > 8:
        rng = np.random.default_rng(seed)
        up = st["bits"] - 8
        L, R = (np.ascontiguousarray((a.astype(np.uint16) << up) | rng.integers(0, 1 << up, a.shape).astype(np.uint16)) for a in (L, R))
        pairs = [(L[j], R[j]) for j in range(st["batch"])]
    return pairs, L, R


TEMPORAL_SHAPE = (48, 20, 16)
SCALED_SHAPE = (97, 41, 2, 16)                     # (W, H, f, D of the small match)
TILE_SHAPE = (77, 32, 16)                          # two row tiles of 16 rows


def scaled_case(batch):
    """a case of tests/scaled_cases.py: the composed call on a batch, another scene per frame"""
    import scaled_cases as SC
    W, H, f, D = SCALED_SHAPE
    return SC.case(f"batch{batch}_{W}x{H}_f{f}", W, H, f, D=D, B=batch, seed=0x5CA1E + 101 * batch)


# -------------------------------------------------------------------------------------- e. tall frames in a large batch
# sgm_post.hip: the chained median runs where (H - 2 + 63) / 64 groups of 64 interior rows exceed MED_WAVES = 8, i.e. from H = 515
# on (a frame of 300 rows has 5 groups and runs the serial kernel); a band is MED_CHAIN_WAVES = 4 groups, the grid is
# dim3(nbands, B).  One round of resident workgroups: a band is a workgroup of 256 threads = 4 waves, a CU holds 32 waves, so at
# most 8 bands per CU and 256 * 8 = 2048 on the chip (registers or LDS can only lower that).  H = 515: 9 groups, 3 bands; the
# smallest B with 3 B > 2048 is 683.
MED_WAVES, MED_CHAIN_WAVES = 8, 4


def median_bands(h):
    """(groups, bands of the chained kernel or 0 where the serial kernel runs)"""
    groups = (h - 2 + 63) // 64
    return groups, (groups + MED_CHAIN_WAVES - 1) // MED_CHAIN_WAVES if groups > MED_WAVES else 0


CHAIN_RESIDENT_MAX = CUS * (WAVES_PER_CU // MED_CHAIN_WAVES)
TALL_CASE = (24, 515, 8, 683)                      # (w, h, d, batch)
TALL_SEED = 0x7A11000


# ------------------------------------------------------------------------------------- f. the opt-in fused sweep (SGM_UPSUM=1)
# sgmd_upsum_rows: Dp = 128, W > H, W >= 64, H >= 4, whole frames, eight paths, P1 >= 0.  320 x 24 keeps enough content at D = 128
# (test_batch_cpu.py asserts the quota); the range is 65 .. 128 for Dp = 128
FUSED_SHAPE = (320, 24, 128)
FUSED_BATCHES = (9, 17)
FUSED_SEED = 0xF05E000


# --------------------------------------------------------------------------------------- g. batch totals past 2^32 cells
# name -> (w, h, d, batch).  sgm_initialize bounds W * H * Dp < 2^32 - 1 per frame and nothing for the batch.
#   fast:  Dp = 128, 510 * 128 * 128 = 8355840 cells per frame; 514 frames are 4294901760 < 2^32, 515 frames 4303257600: B = 515 is
#          the smallest batch past 2^32, and cell 2^32 lies in its last frame
#   dp512: the separate sum / right-view kernels with S and the cost volume; 136 * 64 * 512 = 4456448 cells per frame, cell 2^32 lies
#          in frame 963 of 1024
# Four distinct pairs cycle through the batch, frame j holds pair j % 4; test_batch_cpu.py asserts that the first and the last
# frame, and the frames before, at and behind cell 2^32, are of different pairs.
PAST32 = {"fast": (510, 128, 128, 515), "dp512": (136, 64, 257, 1024)}
PAST32_PAIRS = 4
PAST32_SEED = 0x2320000
CENSUS_FRONT_SLACK_MAX = 1 << 20                   # (an upper bound of the few KB in front of and behind census-right)


def past32_cells(name):
    w, h, d, b = PAST32[name]
    return w * h * padded_stride(d)


def past32_frame_of_cell(name, cell=1 << 32):
    return cell // past32_cells(name)


def past32_pairs(oracle, name):
    w, h, d, _ = PAST32[name]
    return [oracle.synth_pair(w, h, d, frame_seed(PAST32_SEED + 1009 * list(PAST32).index(name), k)) for k in range(PAST32_PAIRS)]


def median_scratch_bytes(w, h, batch):
    """sgmd_median_scratch_bytes of csrc/sgm_post.hip"""
    groups, nbands = median_bands(h)
    if groups <= 0:
        return 16
    nbands = (groups + MED_CHAIN_WAVES - 1) // MED_CHAIN_WAVES
    lag, pf, ne, gpad = 3 * 63, 4, 6, 256                   # MED_LAG = MED_SKEW * 63, MED_PF, MED_NE, MED_GPAD
    tq = (w + lag + 4 * pf - 1) // (4 * pf) * pf
    granules = batch * nbands * (gpad + 4 * tq + 64 + 64 * 4) + batch + 8
    return batch * groups * tq * (ne + 1) * 64 * 16 + granules * 8


def device_bytes(w, h, d, batch, separate_sum=None):
    """What a plain match of whole frames allocates on the device (ensure_buffers, sgm_initialize, ensure_S, ensure_cost of
    csrc/sgm_host.c) -> dict of buffer sizes in bytes.  separate_sum: S and the cost volume exist (Dp = 512 runs the separate
    sum and right-view kernels)."""
    dp = padded_stride(d)
    px = batch * w * h
    sizes = {"images": 2 * px, "census": 2 * 4 * px, "maps": 8 * 4 * px, "lut": 512,
             "planes": batch * 8 * h * w * dp, "extras": batch * 4 * h * dp,
             "median_scratch": median_scratch_bytes(w, h, batch)}
    if dp > 256 if separate_sum is None else separate_sum:
        sizes["S"] = 2 * px * dp
        sizes["cost"] = px * dp
    return sizes


def past32_need(name):
    """device bytes a case of PAST32 needs: the instance's buffers, the census slack, and 1 GiB for the runtime and the test's own
    tensors"""
    w, h, d, b = PAST32[name]
    return sum(device_bytes(w, h, d, b).values()) + 2 * CENSUS_FRONT_SLACK_MAX + (1 << 30)


# ------------------------------------------------------------------------------------------- h. one instance through batches
WALK_SHAPE = MAX_SHAPE
WALK_BATCHES = (17, 5, 1024, 2)                    # plain; plain, shrinks; the maximum, every buffer grows; XCD strips of 4
WALK_SEED = 0x3A1C000


# --------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


_CACHE = {}


def reference(key, make):
    """make() once per process under key, handed out unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def finals(oracle, w, h, d, batch, seed, right_view=False, dmin=0):
    """[(final, raw right view)] * batch of a plain match under option(d): (the right view's pair with right_view)"""
    def make():
        opt = option(d, dmin)
        out = []
        try:
            oracle.set_reference_view(right_view)
            for l, r in frames(oracle, w, h, d, batch, seed)[0]:
                s = oracle.run(l, r, opt)
                out.append((s["final"], s["disp_r"]))
        finally:
            oracle.set_reference_view(False)
        for a, b in out:
            a.setflags(write=False)
            b.setflags(write=False)
        return out
    return reference(("finals", w, h, d, batch, seed, right_view, dmin), make)


QUOTA = 50                                         # finite pixels per frame in `final` (and in the raw right view where compared)


def finite(a):
    return int(np.isfinite(a).sum())
