"""Cases of the scaled match (include/sgm_mi355x.h, sgm_scale_spec), shared by tests/test_scaled_cpu.py (the quotas that make a case
mean something, evaluated on the references alone, without a GPU) and tests/test_gpu_scaled.py (the device against the same
references, bit for bit).  No fixtures; every reference is computed once per process and handed out unchanged.

    COMPOSED   the composed call, option by option            composed(oracle, case) -> its inputs and references
    WALK       the steps of one live instance                 (cases of the same form)
    STREAMS    the three pairs of the stream tests
    ENDS       65535 wide and 65535 tall, composed            (cases of the same form, radius 1)
    PLANTED    the re-search kernel alone on planted inputs   planted_case(case) -> its arrays and references
    quotas(...)                                               what a reference has to show before anything is compared with it

The expected small maps come from expected() of tests/instance_steps.py (the CPU oracle, census_sym_ref, pixels16_ref,
fill_holes_ref, refine_ref on confidence_ref), the full-resolution maps from tests/scaled_ref.py on top of them.

The quotas (set before any device result was seen; none of them is derived from what the device gives):
    finite       more than 0.3 of the pixels are finite
    decided      at least 5 % of the finite pixels differ from the guided upscale alone (radius -1): the re-search decides something
    fraction     at least 1 % of the finite pixels carry a sub-pixel fraction
    refused      with min_disparity 3: some pixels have a candidate p + o that was not admitted
    ties         in the tie cases every window cost A(d) of every candidate of every searched pixel is the same number
Every quota is asserted for every case, with one exception that follows from the spec: where every window cost of every candidate
is ASSERTED equal (the tie cases), den = C(o-1) + C(o+1) - 2 C(o) = 0 at every searched pixel, so no sub-pixel term exists and
"fraction" is waived there, and only there.  Where the spec admits ONE disparity (d_lo == d_hi) it is asserted in addition that at
least 5 % of the pixels were searched and that every searched pixel came out as d_lo.  A case that misses a quota gets another seed,
never a lower quota."""
import numpy as np

import instance_steps as IR
import pixels16_ref as P
import scaled_ref as SR

CENTRE, SYMMETRIC = 0, 1
RADIUS, PENALTY = 3, 1             # SGM_SCALE_DEFAULT_RADIUS / _PENALTY (tests/test_scaled_cpu.py pins them to the header)


# ---- the composed match --------------------------------------------------------------------------------------------------------------

def case(name, W, H, f, D=16, B=1, radius=RADIUS, seed=4242, scene_d=None, speckle=10, **options):
    """options: what step() of tests/instance_steps.py takes (dmin, paths4, kind, window, view, fill, refine, keep, q14,
    bits); scene_d: the disparity range of the synthetic full-resolution pair (default 12 f: inside the small range of 16); speckle:
    min_speckle_area, 0 turns the removal off"""
    return dict(name=name, W=W, H=H, f=f, D=D, B=B, radius=radius, seed=seed + W, scene_d=scene_d or 12 * f, speckle=speckle,
                options=options)


COMPOSED = [
    case("97x41_f2", 97, 41, 2),                                     # one remainder column and one remainder row
    case("131x50_f4_batch2", 131, 50, 4, B=2),                       # remainders 3 and 2; three workgroup columns, the last 3 wide
    case("40x96_f2_tall", 40, 96, 2),                                # W < H at the small shape too
    case("96x40_f2_dmin3", 96, 40, 2, dmin=3, scene_d=38),           # d_lo = 6, d_hi = 37; the scene's disparities reach the top
    case("paths4", 96, 40, 2, paths4=True),
    case("fill", 96, 40, 2, fill=True),
    case("refine", 96, 40, 2, refine=True),
    case("keep_stages", 96, 40, 2, keep=True),
    case("symmetric9x7", 96, 40, 2, kind=SYMMETRIC, window=(9, 7)),
    case("16bit_centre", 96, 40, 2, bits=16),
    case("right_view_fill", 96, 40, 2, view=True, fill=True),
    case("batch3_12bit_f4", 128, 48, 4, B=3, bits=12),
    case("twice_without_reset", 96, 40, 2, q14=True),                # the small sums add (Q14) through the scaled entry point itself
]

# one live instance, step by step
WALK = [
    case("walk1_192x80_f4", 192, 80, 4),                             # small 48x20
    case("walk2_96x40_f2", 96, 40, 2),                               # the same small shape, smaller full buffers
    case("walk3_97x41_f2", 97, 41, 2),
    case("walk4_no_search", 97, 41, 2, radius=-1),                   # the census planes are not needed
    case("walk5_128x48_f2", 128, 48, 2),                             # the small shape grows
    case("walk6_12bit", 96, 40, 2, bits=12),
    case("walk7_batch3_67x19", 67, 19, 2, B=3, D=8, scene_d=12),
    case("walk1_192x80_f4", 192, 80, 4),                             # step 1 again
]

STREAMS = [case("stream_a", 97, 41, 2, seed=611), case("stream_b", 97, 41, 2, seed=733)]
STREAM_SMALL_SEED = 877                                              # the small pair of the plain match behind them

# the ends of the spec, radius 1 so that the numpy reference stays in seconds.  4 columns are fewer than the 5x5 census needs, so the
# tall case matches with the symmetric 3x3 census.  A 4-column frame leaves the winner-take-all about 1 % of its pixels (the ends of
# the range are invalid, and column x sees d <= x only), which the median then removes: the tall case runs with hole filling and
# without speckle removal, and scene and seed are the ones of a small scan (range 10, 12, 14; seeds 1 to 3) that pass "finite".
ENDS = [
    case("65535x16_f2", 65535, 16, 2, D=8, radius=1, scene_d=12, seed=31),
    case("16x65535_f4", 16, 65535, 4, D=8, radius=1, scene_d=10, seed=3, speckle=0, kind=SYMMETRIC, window=(3, 3), fill=True),
]

_CACHE = {}


def scene(W, H, d, frames, bits, seed):
    """full-resolution pairs with structure (the seeded synthetic pair), u16 with random low bits above 8 bits"""
    import soc_project_stereo_matching_amd as S
    rng = np.random.default_rng(seed)
    pairs = [S.synth_pair(W, H, d, seed + k) for k in range(frames)]
    left, right = (np.stack([p[v] for p in pairs]) for v in (0, 1))
    if bits > 8:
        left, right = ((a.astype(np.uint16) << (bits - 8)) | rng.integers(0, 1 << (bits - 8), a.shape).astype(np.uint16) for a in (left, right))
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def step_of(c):
    return IR.step(c["W"] // c["f"], c["H"] // c["f"], c["D"], batch=c["B"], **c["options"])


def option_of(c):
    st = step_of(c)
    opt = IR.option_of(st)
    opt.min_speckle_area = c["speckle"]
    if not c["speckle"]:
        opt.is_remove_speckles = False
    return opt


def full_words(oracle, img, st):
    """the census words of one full-resolution view, by the instance's kind and on the samples as they are"""
    if st["bits"] == 8 and st["kind"] == CENTRE and tuple(st["window"]) == (5, 5):
        return oracle.census(np.ascontiguousarray(img))
    words = P.census(img, st["kind"] == SYMMETRIC, *st["window"])
    assert words.dtype == np.uint32
    return words


def upscaled(oracle, c, st, opt, small, left, right, ls, rs, radius):
    view = bool(st["view"])
    guide, guide_small = (right, rs) if view else (left, ls)
    ref_oth = None, None
    if radius >= 0:
        wl = np.stack([full_words(oracle, a, st) for a in left])
        wr = np.stack([full_words(oracle, a, st) for a in right])
        ref_oth = (wr, wl) if view else (wl, wr)
    with np.errstate(over="ignore"):
        return SR.upscale_batch(small, guide_small, guide, ref_oth[0], ref_oth[1], c["f"], radius, PENALTY, c["f"] * opt.min_disparity,
                                c["f"] * opt.max_disparity - 1, view)


def composed(oracle, c, earlier=()):
    """One composed call of case c alone on a freshly reset instance: dict of the full-resolution pair (left, right [B][H][W]), its
    downscaled twin (ls, rs), the small final map (small), the kept small stages per frame (stages), the full map (want) and the
    guided upscale alone (prior).  With q14 the case is TWO calls without a Reset: first / first_want are the pair and the map of
    the first one, everything else belongs to the second.  earlier: small pairs [(ls, rs)] matched before it on the instance without
    a Reset (not cached)."""
    key = c["name"]
    if not earlier and key in _CACHE:
        return _CACHE[key]
    st, opt = step_of(c), option_of(c)
    f, B, bits = c["f"], c["B"], st["bits"]
    out = {"st": st, "opt": opt}
    before = [list(e) for e in earlier]
    if st["q14"]:
        fl, fr = scene(c["W"], c["H"], c["scene_d"], B, bits, c["seed"] + 53)
        fls, frs = SR.downscale(fl, f), SR.downscale(fr, f)
        first = [IR.expected(oracle, st, opt, fls[k], frs[k])["final"] for k in range(B)]
        out["first"] = (fl, fr)
        out["first_want"] = upscaled(oracle, c, st, opt, np.stack(first), fl, fr, fls, frs, c["radius"])
        before.append((fls, frs))
    left, right = scene(c["W"], c["H"], c["scene_d"], B, bits, c["seed"])
    ls, rs = SR.downscale(left, f), SR.downscale(right, f)
    stages = [IR.expected(oracle, st, opt, ls[k], rs[k], [(a[k], b[k]) for a, b in before] or None) for k in range(B)]
    small = np.stack([s["final"] for s in stages])
    out.update(left=left, right=right, ls=ls, rs=rs, stages=stages, small=small,
               want=upscaled(oracle, c, st, opt, small, left, right, ls, rs, c["radius"]),
               prior=upscaled(oracle, c, st, opt, small, left, right, ls, rs, -1))
    if not earlier:
        _CACHE[key] = out
    return out


def small_pair(oracle, c, seed):
    """a pair at the small shape of case c for a plain match, [B][h][w]"""
    st = step_of(c)
    return scene(st["w"], st["h"], c["D"], c["B"], st["bits"], seed)


def plain(oracle, c, ls, rs, earlier):
    """the final maps [B][h][w] of a plain match of (ls, rs) on case c's instance behind the small pairs `earlier`, no Reset between"""
    st, opt = step_of(c), option_of(c)
    return np.stack([IR.expected(oracle, st, opt, ls[k], rs[k], [(a[k], b[k]) for a, b in earlier] or None)["final"] for k in range(c["B"])])


# ---- the re-search kernel alone ---------------------------------------------------------------------------------------------------------

def planted(rng, W, H, f, frames, bits, inf_share, d_top):
    """a random small map (quarter-pixel values from -1 to d_top / f, so that priors reach past both ends of the admitted range and
    past the pixel's own column), random guides and census words; with more than one frame the LAST frame's census words are one
    constant in both views, so every cost there ties and the tie rules decide"""
    w, h = W // f, H // f
    dt = np.uint16 if bits > 8 else np.uint8
    small = (rng.integers(-4, 4 * d_top // f + 1, (frames, h, w)) / 4.0).astype(np.float32)
    small[rng.random(small.shape) < inf_share] = np.inf
    if inf_share == 0.3:
        small[0, 0, 0] = np.nan                                      # not finite by its bit pattern either
        small[0, -1, -1] = -np.inf
    # few distinct guide values: ties between candidates are the rule, not the exception
    g_small = rng.integers(0, 4, (frames, h, w)).astype(dt) * dt((1 << bits) // 4 - 1)
    g_full = rng.integers(0, 4, (frames, H, W)).astype(dt) * dt((1 << bits) // 4 - 1)
    c_ref = rng.integers(0, 1 << 32, (frames, H, W), dtype=np.uint64).astype(np.uint32)
    c_oth = rng.integers(0, 1 << 32, (frames, H, W), dtype=np.uint64).astype(np.uint32)
    if frames > 1:
        c_ref[-1] = c_oth[-1] = np.uint32(0x5A5A5A5A)
    return small, g_small, g_full, c_ref, c_oth


def extremes(f):
    """small-map values at the ends of float32 and of the prior's clamp: f * 3e38 overflows to +-INF, which is what comes out;
    +-2^20 / f gives the clamp itself, the next float and 1e30 lie beyond it (finite priors no integer holds); -0.0 and a denormal
    keep their bits through prior = f * value"""
    edge = np.float32((1 << 20) / f)
    beyond = np.nextafter(edge, np.float32(np.inf), dtype=np.float32)
    tiny = np.array([0x00000003], np.uint32).view(np.float32)[0]
    return np.array([3e38, -3e38, edge, -edge, beyond, -beyond, 1e30, -1e30, -2.75, -0.0, tiny, -tiny], np.float32)


def pcase(name, W, H, f, radius, bits=8, frames=2, right=False, penalty=1, d_lo=3, d_hi=None, offset=0, values="random", seed=0):
    d_hi = 3 + (W * 2) // 3 if d_hi is None else d_hi
    return dict(name=name, W=W, H=H, f=f, radius=radius, bits=bits, frames=frames, right=right, penalty=penalty, d_lo=d_lo, d_hi=d_hi,
                offset=offset, values=values, seed=seed)


PLANTED = (
    # the instantiations sgm_upscale_k<F, 1> and <F, 2>, both views
    [pcase(f"r{r}_f{f}_{'right' if right else 'left'}", 67, 19, f, r, right=right, bits=12 if f == 4 else 8)
     for r in (1, 2) for f in (2, 4) for right in (False, True)] +
    [pcase("130x9_f2", 130, 9, 2, 3),                                # three workgroup columns, the last 2 pixels wide
     pcase("130x9_f4_right", 130, 9, 4, 2, right=True),
     pcase("9x2_f2", 9, 2, 2, 3, d_hi=9, seed=2),                    # one low-resolution row, fewer rows than a workgroup has
     pcase("odd_frames_f2", 67, 19, 2, 3, frames=3),                 # 1273 pixels per frame (297 small): no frame offset is a multiple of 4
     pcase("odd_frames_f4_12bit", 67, 19, 4, 1, frames=3, bits=12),  # 64 small pixels per frame, 1273 full ones
     pcase("pointers_off_by_one", 67, 19, 2, 3, offset=1),           # every array one element off an aligned allocation
     pcase("pointers_off_by_one_12bit_f4", 70, 23, 4, 2, bits=12, offset=1, right=True),
     pcase("extremes_f2", 67, 19, 2, 3, values="extremes"),
     pcase("extremes_f4_right", 70, 23, 4, 1, values="extremes", right=True),
     pcase("only_0_admitted", 67, 19, 2, 3, d_lo=0, d_hi=0),
     pcase("only_65535_admitted", 67, 19, 2, 3, d_lo=65535, d_hi=65535, penalty=0, values="top"),
     pcase("only_65535_admitted_f4_right", 70, 23, 4, 2, d_lo=65535, d_hi=65535, penalty=0, values="top", right=True),
     pcase("top_three_tie", 67, 19, 2, 3, d_lo=65533, d_hi=65535, penalty=0, values="top")])

# 65535 wide and 65535 tall through the kernel alone
PLANTED_ENDS = [pcase("65535x16_f2", 65535, 16, 2, 1, frames=1, seed=5), pcase("16x65535_f4", 16, 65535, 4, 1, frames=1, right=True, seed=6)]


def planted_case(c):
    """the arrays (small, g_small, g_full, c_ref, c_oth) of a planted case, the full map (want) and the guided upscale alone (prior)"""
    key = "planted " + c["name"]
    if key in _CACHE:
        return _CACHE[key]
    W, H, f = c["W"], c["H"], c["f"]
    rng = np.random.default_rng(W * 1000 + H + 7919 * c["seed"])
    arrays = list(planted(rng, W, H, f, c["frames"], c["bits"], 0.1, c["d_hi"] + 2 * f))
    small = arrays[0]
    if c["values"] == "extremes":
        ext = extremes(f)
        spots = rng.random(small.shape) < 0.15
        small[spots] = ext[rng.integers(0, len(ext), int(spots.sum()))]
        small.reshape(-1)[:len(ext)] = ext                           # each of them at least once
    elif c["values"] == "top":
        # priors 65535 + k, k = -2f-1 .. 2f+1 (exact: 65535 / f has at most two fraction bits): a candidate at 65535 for |k| <= f.
        # Every partner column x -+ d is outside a frame this narrow, so every window term costs 24 whatever the words are
        k = rng.integers(-2 * f - 1, 2 * f + 2, small.shape)
        small[:] = ((65535 + k) / f).astype(np.float32)
        small[rng.random(small.shape) < 0.1] = np.inf
    with np.errstate(over="ignore"):
        want = SR.upscale_batch(*arrays, f, c["radius"], c["penalty"], c["d_lo"], c["d_hi"], c["right"])
        prior = SR.upscale_batch(*arrays[:3], None, None, f, -1, 0, 0, 0, c["right"])
    _CACHE[key] = out = dict(arrays=arrays, want=want, prior=prior)
    return out


# ---- the quotas -----------------------------------------------------------------------------------------------------------------------

def rounded_prior(prior):
    fin = SR.finite_bits(prior)
    return fin, np.rint(np.clip(np.where(fin, prior, np.float32(0)), -SR.PRIOR_MAX, SR.PRIOR_MAX)).astype(np.int64)


def quotas(want, prior, f, d_lo, d_hi, refused=False, ties=None):
    """Asserts what the docstring of this module lists on a reference map and its guided upscale; returns the figures.
    ties: (census_ref, census_oth, radius, right) of a tie case"""
    fin = SR.finite_bits(want)
    n = int(fin.sum())
    bits_w, bits_p = want.view(np.uint32), prior.view(np.uint32)
    with np.errstate(invalid="ignore"):
        fig = {"finite": float(fin.mean()), "decided": float((fin & (bits_w != bits_p)).sum()) / max(n, 1),
               "fraction": float((fin & (want != np.rint(want))).sum()) / max(n, 1)}
    pf, p = rounded_prior(prior)
    searched = pf & (p + f >= d_lo) & (p - f <= d_hi)
    all_tie = False
    if ties is not None:
        c_ref, c_oth, radius, right = ties
        costs = set()
        for k in range(len(want)):
            for o in range(-f, f + 1):
                costs |= set(np.unique(SR.window_costs(c_ref[k], c_oth[k], p[k] + o, radius, right)[searched[k]]).tolist())
        fig["costs"] = sorted(costs)
        assert len(costs) == 1, fig
        all_tie = True                                               # asserted: den = 0 at every searched pixel, no sub-pixel term exists
    assert fig["finite"] > 0.3, fig
    assert fig["decided"] >= 0.05, fig
    assert fig["fraction"] >= 0.01 or all_tie, fig
    if d_lo == d_hi:                                                 # in addition: the one admitted disparity is what the searched pixels get
        fig["searched"] = float(searched.mean())
        assert fig["searched"] >= 0.05 and (want[searched] == d_lo).all(), fig
    if refused:
        fig["refused"] = int((searched & ((p - f < d_lo) | (p + f > d_hi))).sum())
        assert fig["refused"] > 0, fig
    return fig


def composed_quotas(c, r):
    opt = r["opt"]
    return quotas(r["want"], r["prior"], c["f"], c["f"] * opt.min_disparity, c["f"] * opt.max_disparity - 1, refused=opt.min_disparity > 0)


def planted_quotas(c, r):
    ties = (r["arrays"][3], r["arrays"][4], c["radius"], c["right"]) if c["values"] == "top" else None
    return quotas(r["want"], r["prior"], c["f"], c["d_lo"], c["d_hi"], ties=ties)
