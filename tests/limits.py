"""The limits sgm_initialize admits, as lists of cases: min_disparity up to 65535 - D, frames 65535 wide or tall, padded cost
volumes W * H * Dp with bit 31 set in the cell offset, and the ends of the option fields.  A plain helper module, no fixtures;
shared by tests/golden/make_golden_limits.py (the reference's digests -> tests/golden/limits.json), test_limits_cpu.py (the
oracle against them) and test_gpu_limits.py (the library against the oracle / the digests).  DESIGN.md section 2 has the table
of the limits and the test that reaches each."""
import functools
import json
import os

import numpy as np

import wta_classes as WC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLDEN, "limits.json")) as f:
        return json.load(f)


def golden_case(name):
    return golden()["cases"][name]


# ------------------------------------------------------------------------------------------------ A. large minimum disparity
# (w, h, dmin, D); the padded disparity stride of the device kernels in the comment.  The lowest frame is 12 rows, not 8: four
# planted bands need 3 rows each (wta_classes.planted_pair).
DMIN_IN_RANGE = [(160, 24, 100, 16),        # 32
                 (700, 24, 500, 64),        # 64
                 (1000, 16, 300, 128),      # 128
                 (900, 12, 200, 192),       # 192
                 (900, 12, 256, 256),       # 256
                 (1400, 12, 600, 512)]      # 512: the separate sum / right-view kernels
# dmin + D reaches, touches and passes W; then far outside, and the last value the 16-bit fields hold
DMIN_OUT = [(160, 24, dmin, 16) for dmin in (152, 159, 160, 161, 5000, 65519)]
DMIN_CASES = DMIN_IN_RANGE + DMIN_OUT
DMIN_EXTRA = [(160, 24, 100, 16), (1000, 16, 300, 128)]     # the shapes that run every mode
DMIN_QUOTA = 200                                            # finite pixels in `final` and in the raw right view (in-range shapes)
DMIN_OPTION = dict(min_speckle_area=10, is_check_unique=True)


def dmin_name(c):
    return f"dmin_{c[0]}x{c[1]}_d{c[2]}+{c[3]}"


def dmin_ks(D):
    """Planted indices k = d - dmin: both ends of the range, the middle, one 16-lane boundary (index 16, the first lane of the
    second group; D = 16 has one group, whose last lane is the end of the range already)."""
    ks = [0, D - 1, D // 2] + ([16] if D > 16 else [])
    assert len(set(ks)) == len(ks)
    return ks


def dmin_seed(c, frame=0):
    return 0x11A000 + 97 * DMIN_CASES.index(tuple(c)) + 7 * frame


def dmin_option(c, **kw):
    from oracle.pyoracle import default_option
    return default_option(c[2] + c[3], c[2], **dict(DMIN_OPTION, **kw))


def dmin_pair(synth, c, frame=0):
    w, h, dmin, D = c
    return WC.planted_pair(synth, w, h, dmin, D, dmin_seed(c, frame), dmin_ks(D))


# ------------------------------------------------------------------------------------------- B. frames 65535 wide or tall
# (w, h, dmin, D, batch)
WIDE_CASES = [(65535, 6, 0, 8, 1), (65535, 8, 3, 16, 2), (6, 65535, 0, 8, 1), (8, 65535, 0, 16, 2),
              (40000, 12, 0, 64, 1), (12, 40000, 0, 64, 1),          # thousands of diagonal wraps with content
              (65535, 5, 0, 128, 1),                                 # also under SGM_UPSUM=1
              # the degenerate ones.  1 x 65535 is refused (REFUSALS below): one pixel wide, the anomalous lines stay on one row
              # and the table of their visits grows with H^2; 1 x 4096 is the tallest such frame admitted
              (65535, 1, 0, 8, 1), (1, 4096, 0, 8, 1), (65535, 3, 0, 8, 1), (3, 65535, 0, 8, 1),
              (32768, 8, 0, 8, 1), (32769, 8, 0, 8, 1), (8, 32769, 0, 8, 1)]     # the reference's speckle boundary
WIDE_OPTION = dict(min_speckle_area=10)
# the shapes of the crafted post-filter maps and of the restated int16 rule
POST_SHAPES = [(65535, 8), (8, 65535)]
POST_MAPS = ("flat", "ramp", "stripes_v", "stripes_h", "holes", "noise_thr")
POST_AREAS = (1, 50, 65535)
INT16_RULE_CASES = [(65535, 8, 3, 16, 2), (8, 65535, 0, 16, 2), (32769, 8, 0, 8, 1), (8, 32769, 0, 8, 1)]


def wide_name(c):
    return f"wide_{c[0]}x{c[1]}_d{c[2]}+{c[3]}_b{c[4]}"


def wide_seed(c, frame=0):
    return 0x31DE00 + 131 * WIDE_CASES.index(tuple(c)) + 7 * frame


def wide_option(c):
    from oracle.pyoracle import default_option
    return default_option(c[2] + c[3], c[2], **WIDE_OPTION)


def wide_pair(synth, c, frame=0):
    return synth(c[0], c[1], c[3], wide_seed(c, frame))


def beyond_int16(w, h):
    """The reference's RemoveSpeckles cuts components where a coordinate passes 32767 (reference_speckles below)."""
    return w > 32768 or h > 32768


def reference_speckles(disp, min_area, diff=1.0):
    """The reference's RemoveSpeckles (SemiGlobalMatching.c:585-642) restated with its int16_t neighbour coordinates
    (:618-620): a neighbour whose row or column, computed as row + r / col + c, does not fit an int16_t wraps negative and is
    rejected.  A pixel in a row or column >= 32768 therefore reaches no neighbour but those in row / column 32767 (from 32768,
    one step down), and nobody in row / column 32767 reaches it: components are grown along directed links, in raster order
    of their seeds, exactly as the C does.  Where W, H <= 32768 this is the plain 8-connected component rule of the oracle."""
    h, w = disp.shape
    out = np.array(disp, np.float32, copy=True)
    flat = out.reshape(-1)
    valid = ~np.isinf(flat)
    vals = flat.astype(np.float64).tolist()            # the difference of two float32 values is exact in float64 ...
    visited = (~valid).tolist()                        # an invalid pixel is never entered
    diff = float(np.float32(diff))
    steps = [(r, c) for r in (-1, 0, 1) for c in (-1, 0, 1) if (r, c) != (0, 0)]
    kill = []
    for p in np.flatnonzero(valid).tolist():
        if visited[p]:
            continue
        visited[p] = True
        comp = [p]
        i = 0
        while i < len(comp):
            q = comp[i]
            i += 1
            row, col = divmod(q, w)
            base = vals[q]
            for r, c in steps:
                rr, cc = row + r, col + c
                if rr > 32767 or cc > 32767 or rr < 0 or cc < 0 or rr >= h or cc >= w:      # (int16_t) wraps negative past 32767
                    continue
                n = rr * w + cc
                if visited[n]:
                    continue
                delta = abs(vals[n] - base)
                # ... and the C rounds it to float before it compares: a difference just above the threshold may round onto it
                if delta <= diff or (delta <= diff * 1.000001 and float(np.float32(delta)) <= diff):
                    visited[n] = True
                    comp.append(n)
        if len(comp) < min_area:
            kill.extend(comp)
    flat[kill] = INF
    return out


# ------------------------------------------------------------------------ C. volumes with bit 31 set in the cell offset
# name -> (w, h, D, seed); default options.  Dp = 512 / 256 / 128 / 128: W * H * Dp passes 2^31 while the real volume W * H * D
# stays below it (the compiled reference indexes with int).
BIG_CASES = {"dp512": (3000, 2600, 257, 0xB16C0001),
             "dp256": (4200, 2500, 193, 0xB16C0002),
             "dp128_wide": (6000, 3600, 65, 0xB16C0003),
             "dp128_tall": (3600, 6000, 65, 0xB16C0004)}
BIG_ALL_STAGES = ("dp512", "dp256")                 # the Dp = 128 cases compare all stages but `cost` and `aggr`
# with all nine stages dp512 took 11.04 s beside 5.50 s of test_full_size_digests[c3_middlebury_2880x1988_d256] in the same run:
# past twice that, so its 2 GB `cost` read-back is dropped (dp256 keeps it); `aggr`, whose offsets pass 2^31, stays.  Without
# `cost`: 8.48 s beside 4.75 s
BIG_WITHOUT_COST = ("dp512",)
# (w, h, D, accepted): exactly 2^32 padded cells, one column less, a range past the largest, the 31-bit pixel guard; one pixel
# wide: the per-row table of anomalous-line visits has H x H (H even) or H x (H + 1) (H odd) entries, admitted up to 2^24
REFUSALS = [(4096, 2048, 257, False), (4095, 2048, 257, True), (64, 20, 513, False), (65535, 65535, 8, False),
            (1, 65535, 8, False), (1, 4097, 8, False), (1, 4096, 8, True)]


def padded_stride(D):
    """pick_dpl of csrc/sgm_host.c, as DESIGN.md documents it: 16 lanes of 2, 4, 8, 12, 16 or 32 disparities."""
    for dp in (32, 64, 128, 192, 256, 512):
        if D <= dp:
            return dp
    raise ValueError(D)


# -------------------------------------------------------------------------------------------- D. ends of the option fields
OPTION_SHAPE = (64, 20, 0, 16)
OPTION_SEED = 0x0E7D5
# name -> (option overrides, honor_num_paths, defined by the reference)
OPTION_ENDS = {"ratio_0": (dict(uniqueness_ratio=0.0), False, True),
               "ratio_1.5": (dict(uniqueness_ratio=1.5), False, True),
               "ratio_-1": (dict(uniqueness_ratio=-1.0), False, True),
               "lr_-1": (dict(lrcheck_thres=-1.0), False, True),
               "lr_1e30": (dict(lrcheck_thres=1e30), False, True),
               "speckle_0": (dict(min_speckle_area=0), False, True),
               "paths_0": (dict(num_paths=0), False, True),
               "paths_3": (dict(num_paths=3), False, True),
               "paths_255": (dict(num_paths=255), False, True),
               # the reference never reads num_paths; honouring it is this project's extension, and anything but 4
               # means all eight paths: the expected values are the reference's for eight paths all the same
               "paths_0_honored": (dict(num_paths=0), True, True),
               "paths_3_honored": (dict(num_paths=3), True, True),
               "paths_255_honored": (dict(num_paths=255), True, True)}
# cases whose expected values the oracle alone defines, with the reason (none of part D: see above)
ORACLE_ONLY = {}
# cases whose digests are the compiled reference's although its C leaves the result undefined: the reason, stored with the case
_UB = ("(uint16_t)((float)m1 * (1 - uniqueness_ratio)), SemiGlobalMatching.c:422, leaves the range of uint16_t (%s): undefined in C. "
       "The digests are what the reference compiled by gcc for x86-64 gives (cvttss2si, then the low 16 bits); the oracle and the "
       "device ((unsigned short)(int), csrc/sgm_wta.hpp) restate that conversion and agree with it.")
OPTION_NOTES = {"ratio_1.5": _UB % "negative products", "ratio_-1": _UB % "products of 2 * m1 past 65535"}


def option_pair(synth):
    w, h, dmin, D = OPTION_SHAPE
    return WC.planted_pair(synth, w, h, dmin, D, OPTION_SEED, dmin_ks(D))


def option_of(name):
    from oracle.pyoracle import default_option
    kw = dict(min_speckle_area=10)
    kw.update(OPTION_ENDS[name][0])
    return default_option(OPTION_SHAPE[2] + OPTION_SHAPE[3], OPTION_SHAPE[2], **kw)
