"""ONE instance kept alive across changing shapes, batches and options -- needs an MI355X.

A product caller re-initialises the same instance to another resolution, shrinks the batch, switches the census, turns filling,
refinement or rectification on and off.  csrc/sgm_host.c is written for that: its buffers only grow, some are zero-filled only
when they are allocated (d_S, the median scratch, the scratch of the fused last sweep), the path tables and the census block map
are cached under a key, S is cleared lazily.  Every one of these outlives a shape.  Here one instance is driven through a list of
steps and, after EVERY step, compared with what a fresh computation of that step alone gives: the CPU oracle (explicit instances
have no census history, tests/test_census_history.py), and for what the reference does not have the checkers the feature's own
GPU test uses (census_sym_ref, fill_holes_ref, refine_ref on confidence_ref, rectify_ref; composed in tests/instance_steps.py).  Compared: the final map (both maps of
sgm_match_both, the confidence of sgm_match_confidence), the raw right-view map and the aggregated costs read back (re-created
where the fused kernels never stored them).  Tolerance 0, bit patterns.  tests/test_instance_reuse_cpu.py checks on the stand-in
device what re-initialises each piece of retained state; NOTES.md section 20 has the table."""
import numpy as np
import pytest

from instance_steps import CENTRE, SYMMETRIC, apply, expected, option_of, step   # (tests/instance_steps.py; importers take them from here too)
from oracle.pyoracle import default_option

pytestmark = pytest.mark.gpu


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
    if g.dtype == np.float32:
        g, w = g.view(np.uint32), w.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {first}: gpu={got[first]} want={want[first]}")


def frames_of(oracle, st, seed):
    pairs = [oracle.synth_pair(st["w"], st["h"], st["d"], seed + 7 * j) for j in range(st["batch"])]
    return pairs, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def run_match(inst, st, L, R):
    """the step's entry point on [B][H][W] images -> dict of [B][H][W] outputs"""
    b = st["batch"]
    if b == 1:
        L, R = L[0], R[0]
    shape = (b, st["h"], st["w"])
    if st["entry"] == "confidence":
        got = inst.match_confidence(L, R)
        assert got is not None
        return {"final": got[0].reshape(shape), "conf": got[1].reshape(shape)}
    if st["entry"] == "both":
        got = inst.match_both(L, R)
        assert got is not None
        return {"final": got[0].reshape(shape), "final_r": got[1].reshape(shape)}
    got = inst.match(L, R)
    assert got is not None
    return {"final": got.reshape(shape)}


def drive(oracle, inst, steps, what, seed, after=None):
    """ONE instance through the steps; after every step the comparison with that step computed alone"""
    for k, st in enumerate(steps):
        tag = f"{what} step {k} ({st['w']}x{st['h']} d{st['d']} dmin{st['dmin']} batch {st['batch']})"
        opt = option_of(st)
        apply(inst, st)
        assert inst.reset(st["w"], st["h"], opt), tag
        pairs, L, R = frames_of(oracle, st, seed + 101 * k)
        out = run_match(inst, st, L, R)
        prev = None
        if st["q14"]:                                         # a second match without Reset: its sums add to the first's
            prev = pairs
            pairs, L, R = frames_of(oracle, st, seed + 101 * k + 53)
            out = run_match(inst, st, L, R)
        if after:
            after(inst, k, tag)
        for j, (l, r) in enumerate(pairs):
            want = expected(oracle, st, opt, l, r, None if prev is None else prev[j])
            inst.select_frame(j)
            for name in ("final", "final_r", "conf"):
                if name in want:
                    assert_same(out[name][j], want[name], f"{tag} frame {j}: {name}")
            assert_same(inst.read_stage("disp_r"), want["disp_r"], f"{tag} frame {j}: right-view map")
            for name in ("disp_l", "after_lr", "after_speckle"):
                if name in want and st["entry"] != "both":    # (a both-views match keeps them for both views: its own test)
                    assert_same(inst.read_stage(name), want[name], f"{tag} frame {j}: kept stage {name}")
            assert_same(inst.read_stage("aggr"), want["aggr"], f"{tag} frame {j}: aggregated costs")


def new_instance(monkeypatch, env):
    import soc_project_stereo_matching_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, v)                              # read at sgm_create
    return S.SGMInstance(0)


# ---- the shape ladder, one sequence per mode --------------------------------------------------------------------------------

# (W, H, D, dmin): the start; a shrink; tall (W < H: the diagonal planes are cleared per match, the ghost cells of the reused
# planes); a frame the 5x5 census writes nothing of; wide with a padded range of 128; the first shape again, everything in between
LADDER = [(96, 64, 64, 0), (48, 20, 16, 0), (33, 70, 32, 3), (5, 9, 8, 0), (200, 24, 128, 0), (96, 64, 64, 0)]

MODES = {
    "default": ({}, {}),
    "separate_sum": ({"SGM_FUSED_WTA": "0"}, {}),
    "plain_step": ({"SGM_AGG_FAST": "0"}, {}),
    "keep_stages": ({}, dict(keep=True)),
    "batch3": ({}, dict(batch=3)),                            # 8 lanes per pixel, 16-lane horizontals
    "paths4": ({}, dict(paths4=True)),
    "symmetric7x7": ({}, dict(kind=SYMMETRIC, window=(7, 7))),
    "centre9x7": ({}, dict(window=(9, 7))),                   # u64 words, the volume-fed aggregation
    "confidence": ({}, dict(entry="confidence")),
    "both": ({}, dict(entry="both")),
    "fill": ({}, dict(fill=True)),
    "refine": ({}, dict(refine=True)),
}


def ladder(kw):
    shapes = LADDER
    if kw.get("window") == (9, 7) and kw.get("kind", CENTRE) == CENTRE:
        shapes = [s for s in LADDER if s[0] > 9 and s[1] > 7]  # the shapes that admit the window
    return [step(w, h, d, dmin=dmin, **kw) for (w, h, d, dmin) in shapes]


@pytest.mark.parametrize("mode", list(MODES))
def test_shape_ladder(oracle, monkeypatch, mode):
    env, kw = MODES[mode]
    inst = new_instance(monkeypatch, env)
    try:
        drive(oracle, inst, ladder(kw), mode, 0x1AD0 + 1009 * list(MODES).index(mode))
    finally:
        inst.close()


@pytest.mark.parametrize("mode", ["default", "separate_sum", "batch3"])
def test_match_without_reset_on_every_step_of_the_ladder(oracle, monkeypatch, mode):
    """Q14 after a shrink: d_S is kept, full of the larger shape's sums, and cleared lazily.  On every step a second match without
    Reset, against an oracle that did Reset + Match + Match on that step alone."""
    env, kw = MODES[mode]
    inst = new_instance(monkeypatch, env)
    try:
        drive(oracle, inst, ladder(dict(kw, q14=True)), mode + " q14", 0x1E14 + 1009 * list(MODES).index(mode))
    finally:
        inst.close()


# ---- switches on a live instance at a fixed shape -----------------------------------------------------------------------------

def _identity(w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x, y


def _maps(kind, w=96, h=64):
    x, y = _identity(w, h)                                    # (the identity and shifted maps of tests/test_gpu_rectify.py)
    return {"identity": (x, y, x, y), "shift": (x + 3, y - 2, x + 3, y - 2), "other": (x + 2, y + 1, x - 1, y)}[kind]


def _at(**kw):
    return step(96, 64, 64, **kw)


SWITCHES = {
    "batch_3_1_2_3": [_at(batch=3), _at(batch=1), _at(batch=2), _at(batch=3)],
    "penalties": [_at(), _at(pen=(60, 250)), _at()],
    "paths_8_4_8": [_at(), _at(paths4=True), _at()],
    "census": [_at(kind=SYMMETRIC, window=(9, 7)), _at(), _at(window=(9, 7)), _at()],
    "reference_view": [_at(), _at(view=True), _at()],
    "fill_on_off": [_at(fill=True), _at()],
    "refine_on_off": [_at(refine=True), _at()],
    # sgm_set_rectify(NULL maps) clears them (include/sgm_mi355x.h): on, on with shifted maps, off, on with other maps
    "rectify": [_at(rect="identity"), _at(rect="shift"), _at(), _at(rect="other")],
    "keep_stages_on_off": [_at(keep=True), _at()],
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_switch_on_a_live_instance(oracle, monkeypatch, name):
    steps = [dict(st, rect=_maps(st["rect"]) if st["rect"] else None) for st in SWITCHES[name]]
    inst = new_instance(monkeypatch, {})
    try:
        drive(oracle, inst, steps, name, 0x5317 + 1009 * list(SWITCHES).index(name))
    finally:
        inst.close()


# ---- row tiles ----------------------------------------------------------------------------------------------------------------

def _tile(inst, rows, w, h, opt, dl, dr, disp, import_from, export_to):
    """One visit of the instance to a tile: Reset to its rows, the horizontal lines, both sweeps in the order the hand-overs allow.
    import_from / export_to: {forward: buffer}.  A tile whose backward hand-over does not exist yet stops after its forward
    sweep (finish=False) and is visited again."""
    import torch
    assert inst.set_rows(*rows) and inst.reset(w, h, opt)
    torch.cuda.synchronize()
    assert inst.tile_begin(dl.data_ptr(), dr.data_ptr())
    for forward in (True, False):
        if forward in import_from:
            assert inst.tile_import_boundary(forward, import_from[forward].data_ptr())
        elif (rows[0] > 0) if forward else (rows[1] < h):
            return False                                      # the neighbour has not been there yet
        assert inst.tile_sweep(forward)
        if forward in export_to:
            assert inst.tile_export_boundary(forward, export_to[forward].data_ptr())
    assert inst.tile_finish(disp.data_ptr()) and inst.synchronize()
    return True


def test_row_tiles_of_one_frame_on_one_instance(oracle, monkeypatch):
    """The top tile and the bottom tile of a frame on ONE instance (the tile calls of tests/test_gpu_tiling.py, the hand-over
    buffers standing in for the neighbour): top (forward sweep, its hand-over out), bottom (both sweeps, finished), top again
    (now with the bottom's hand-over, finished) -- the planes, the census words and the census block map are those of the other
    tile each time.  The gathered map after the whole-frame post pass is the single-instance result bit for bit.  Then whole
    frames again on the same instance, then another width with the same row split (the block map's key changes in W only)."""
    import torch
    monkeypatch.setenv("SGM_DEBUG_POISON_CENSUS", "1")        # a census word nobody computed must not pass as stale data
    inst = new_instance(monkeypatch, {})
    try:
        for (w, h, d) in ((130, 48, 64), (77, 48, 64)):
            opt = default_option(d, min_speckle_area=10)
            left, right = oracle.synth_pair(w, h, d, 0x7113 + w)
            want = oracle.run(left, right, opt)
            dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            # (a map per tile, as the engines of tests/test_gpu_tiling.py have: only the tile's rows of it count)
            disp, disp_b = (torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(2))
            top, bottom = (0, h // 2), (h // 2, h)
            assert inst.set_rows(*top) and inst.reset(w, h, opt)
            fwd = torch.empty(inst.tile_boundary_bytes(), dtype=torch.uint8, device="cuda")
            bwd = torch.empty_like(fwd)
            assert not _tile(inst, top, w, h, opt, dl, dr, disp, {}, {True: fwd})
            assert inst.synchronize()
            assert _tile(inst, bottom, w, h, opt, dl, dr, disp_b, {True: fwd}, {False: bwd})
            assert_same(inst.read_stage("aggr")[h // 2:], want["aggr"][h // 2:], f"{w}x{h}: S of the bottom tile")
            assert _tile(inst, top, w, h, opt, dl, dr, disp, {False: bwd}, {})
            assert_same(inst.read_stage("aggr")[:h // 2], want["aggr"][:h // 2], f"{w}x{h}: S of the top tile")
            disp[h // 2:] = disp_b[h // 2:]
            torch.cuda.synchronize()
            assert inst.tile_post(disp.data_ptr()) and inst.synchronize()
            assert_same(disp.cpu().numpy(), want["final"], f"{w}x{h}: the gathered map")
            # whole frames again
            assert inst.set_rows(0, 0) and inst.reset(w, h, opt)
            assert_same(inst.match(left, right), want["final"], f"{w}x{h}: a plain match after the tiles")
            assert_same(inst.read_stage("aggr"), want["aggr"], f"{w}x{h}: S of the plain match")
    finally:
        inst.close()


# ---- the fused last sweep -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [3, 1])
def test_fused_sweep_across_shapes_and_batches(oracle, monkeypatch, rows):
    """SGM_UPSUM=1: the kernel's progress words sit behind the hand-over rows of its scratch, at an offset that depends on batch,
    width and range, and the scratch is kept when the geometry shrinks -- the words then lie where the larger shape's hand-over
    bytes were.  A stale word whose top bit is clear reads as "ahead", and a row group would read a hand-over row before the
    group below has written it.  The host zero-fills the scratch and restarts the generation whenever the geometry differs from
    the launch before.  The stale-word failure is a RACE: a group that arrives late reads the right row anyway, so this test can
    pass on a host without the fix.  The deterministic proof is tests/test_instance_reuse_cpu.py on the stand-in device; this
    one checks that the results are right with the fix in, at 3 rows per workgroup and at 1 (every hand-over through global
    memory).  The first frames are the tallest, so that many row groups of the later ones meet words of the first."""
    steps = [step(640, 60, 128, batch=3), step(300, 40, 128, batch=3), step(161, 20, 128, dmin=3, batch=3),
             step(161, 20, 128, dmin=3, batch=2), step(130, 16, 128, batch=2), step(640, 60, 128, batch=2)]
    env = {"SGM_UPSUM": "1"}
    if rows != 3:
        env["SGM_UPSUM_ROWS"] = str(rows)
    inst = new_instance(monkeypatch, env)

    def fused(i, k, tag):
        assert i.fused_sweep_rows() == rows, tag

    try:
        drive(oracle, inst, steps, f"fused sweep, {rows} rows", 0x0F5E + rows, after=fused)
    finally:
        inst.close()


# ---- the median's granule rows --------------------------------------------------------------------------------------------------

def test_median_granules_across_heights(oracle):
    """Frames of more than 512 interior rows run the median as a chain of bands (4 waves x 64 rows each) that hand their last row
    down through tagged granules in the median scratch (csrc/sgm_post.hip: med_chain needs more than 8 groups of 64 interior rows,
    med_granules places the granule rows behind B * groups * Tq result tiles).  The scratch is zeroed once, when it is allocated;
    the granule rows' offset depends on W and H.  H = 515 is the smallest height with a chain (9 groups, 3 bands); 1100 rows give
    18 groups and 5 bands, so the granule rows of the shorter frame lie in the taller one's input tiles, and those of the
    tall frame's second visit in what the shorter left.  Widths 40 and 24 move the rows within the scratch and cost little.
    Crafted maps through the post-filter entry (speckle removal off), as tests/test_gpu_parity.py does for tall frames."""
    import torch
    import soc_project_stereo_matching_amd as S
    inst = S.SGMInstance(0)
    try:
        for k, (w, h) in enumerate([(40, 1100), (24, 515), (40, 1100), (40, 515), (24, 1100)]):
            assert inst.reset(w, h, S.default_option(16, is_remove_speckles=False))
            rng = np.random.default_rng(0x3ED + k)
            for rep in range(2):
                m = rng.integers(0, 64, (h, w)).astype(np.float32) + rng.integers(0, 4, (h, w)).astype(np.float32) / 4
                m[rng.random((h, w)) < 0.2] = np.inf
                t = torch.from_numpy(m.copy()).cuda()
                torch.cuda.synchronize()
                assert inst.tile_post(t.data_ptr()) and inst.synchronize()
                assert_same(t.cpu().numpy(), oracle.median(m.copy()), f"step {k} ({w}x{h}) map {rep}")
    finally:
        inst.close()
