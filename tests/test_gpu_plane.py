"""Planes in a point list on the device (extension; include/sgm_mi355x.h, sgm_plane_spec) against the numpy restatement
tests/plane_ref.py -- needs an MI355X.  Tolerance 0 everywhere: candidates, votes, the best plane, the sums, the labels and the
fit's planes, sums and stats are compared byte by byte; every output sits between margins of 0xA5 and the inputs are compared
unchanged.  Records are 16-byte aligned only, the sums 8-byte aligned only, the labels start at an odd address."""
import numpy as np
import pytest

import cloud_ref as CR
import geometry_large as GL
import mesh_ref as MR
import plane_ref as PR
import volume_ref as VR
from test_gpu_raycast import MARGIN, Between
from test_gpu_volume import c_source, c_volume
from test_plane_cpu import (FLOOR, NOISE, WALL, c_spec, collinear_records, coplanar_records, edge_records, planted_scene, planted_spec,
                            recovered, sums_edge_case)
from test_volume_cpu import noisy_scene

pytestmark = pytest.mark.gpu

THREADS, RECORDS, MAX_BLOCKS = (GL.constant("sgm_plane.hip", n) for n in ("PLANE_THREADS", "PLANE_RECORDS", "PLANE_MAX_BLOCKS"))
WAVE_TRIP = 64 * RECORDS                                          # the records a wave of the vote holds at a time
VOTE_LAP = MAX_BLOCKS * THREADS * RECORDS                         # one lap of the vote's grid
LAP = MAX_BLOCKS * THREADS                                        # one lap of the sums' and the labels' grid
f32 = np.float32


class Shifted(Between):
    """Between, `shift` bytes (at most 16) further into its allocation: 16 for a pointer that is 16-byte aligned and no more, 8 for the
    sums, 1 for the labels"""
    def __init__(self, nbytes, data=None, shift=0):
        import torch
        assert 0 <= shift <= 16
        self.torch, self.nbytes = torch, nbytes
        self.off = MARGIN + shift
        self.hold = torch.full((nbytes + 2 * MARGIN + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.hold.data_ptr() % 64 == 0
        if data is not None:
            self.hold[self.off:self.off + nbytes].copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8)))


class Device:
    """a list on the device -- capacity records of which the count word admits n -- and room for every output"""
    def __init__(self, rec, k, n=None, labels=None):
        self.rec_host = np.ascontiguousarray(rec)
        self.capacity = len(rec)
        self.n = self.capacity if n is None else n
        self.rec = Shifted(16 * self.capacity, self.rec_host, 16)
        self.count = None if n is None else Shifted(4, np.array([n], np.uint32), 4)
        self.labels_host = None if labels is None else np.array(labels, np.uint8)
        self.labels = None if labels is None else Shifted(self.capacity, self.labels_host, 1)
        self.marks = Shifted(self.capacity, np.zeros(self.capacity, np.uint8) if labels is None else self.labels_host, 1)
        self.k = k
        self.planes, self.best, self.sums = Shifted(32 * k, shift=16), Shifted(32, shift=16), Shifted(80, shift=8)

    ptr = staticmethod(lambda b: None if b is None else b.ptr)

    def chain(self, inst, sp, label, value=9):
        """votes, best, sums at the best plane, labels of the best plane: queued back to back, one synchronisation at the end"""
        cs = c_spec(sp)
        self.torch_sync()
        a = (self.rec.ptr, self.capacity, self.ptr(self.count))
        assert inst.plane_votes(cs, *a, self.ptr(self.labels), self.planes.ptr), label
        assert inst.plane_best(self.planes.ptr, self.k, self.best.ptr), label
        assert inst.plane_sums(cs, *a, self.ptr(self.labels), self.best.ptr, self.sums.ptr), label
        assert inst.plane_label(cs, *a, self.best.ptr, value, self.marks.ptr), label
        assert inst.synchronize(), label
        out = (self.planes.read(label + " planes").view(PR.PLANE_DTYPE).copy(), self.best.read(label + " best").view(PR.PLANE_DTYPE)[0].copy(),
               self.sums.read(label + " sums").view(np.int64).copy(), self.marks.read(label + " labels").copy())
        self.unchanged(label)
        return out

    def unchanged(self, label):
        assert self.rec.read(label + " records").tobytes() == self.rec_host.tobytes(), f"{label}: the records are only read"
        assert self.count is None or self.count.read(label + " count").view(np.uint32)[0] == self.n, f"{label}: the count is only read"
        assert self.labels is None or self.labels.read(label + " labels in").tobytes() == self.labels_host.tobytes(), f"{label}: labels are only read"

    def torch_sync(self):
        self.rec.torch.cuda.synchronize()


def check(inst, sp, rec, label, n=None, labels=None, value=9):
    """the chain against the restatement; returns the restatement's (planes, best, sums, labels)"""
    dev = Device(rec, sp.hypotheses, n, labels)
    planes, best, sums, marks = dev.chain(inst, sp, label, value)
    m = dev.n
    want_planes = PR.votes(sp, rec, m, labels)
    want_best = PR.best(want_planes)
    want_sums = PR.sums(sp, rec, m, labels, want_best)
    want_marks = PR.label(sp, rec, m, want_best, value, np.zeros(len(rec), np.uint8) if labels is None else labels)
    bad = [k for k in range(sp.hypotheses) if planes[k].tobytes() != want_planes[k].tobytes()]
    assert not bad, f"{label}: {len(bad)} of {sp.hypotheses} candidates differ, first {bad[0]}: {planes[bad[0]]} != {want_planes[bad[0]]}"
    assert best.tobytes() == want_best.tobytes(), f"{label}: best {best} != {want_best}"
    assert sums.tolist() == want_sums.tolist(), f"{label}: sums {sums.tolist()} != {want_sums.tolist()}"
    assert np.array_equal(marks, want_marks), f"{label}: {(marks != want_marks).sum()} labels differ"
    return want_planes, want_best, want_sums, want_marks


def fit(inst, sp, rec, label, n=None, labels=None):
    """sgm_plane_fit against the restatement, traces included; returns the restatement's (plane, stats)"""
    dev = Device(rec, 1, n, labels)
    dev.torch_sync()
    got = inst.plane_fit(c_spec(sp), dev.rec.ptr, dev.capacity, dev.ptr(dev.count), dev.ptr(dev.labels), trace=True)
    assert got is not None, label
    dev.unchanged(label)
    want = PR.fit(sp, rec, dev.n, labels)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], f"{label}: {got[0]} {got[1]} != {want[0]} {want[1]}"
    assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes(), f"{label}: the traces differ"
    return want[0], want[1]


@pytest.fixture(scope="module")
def inst():
    import soc_project_stereo_matching_amd as S
    i = S.SGMInstance(0)                                          # never initialised: the planes need no shape
    yield i
    i.close()


def slab(n, seed=1):
    """n records around the plane 0.6 y + 0.8 z = 1, two thirds within 0.01 of it"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
    off = np.where(rng.random(n) < 0.67, rng.uniform(-0.01, 0.01, n), rng.uniform(-1, 1, n))
    return PR.records_of(np.stack([u, 0.8 * v + 0.6 * (1 + off), -0.6 * v + 0.8 * (1 + off)], 1))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, WAVE_TRIP + 1, THREADS * RECORDS + 1])
def test_small_lists_through_a_count_word(inst, n):
    """n records admitted by the count word, of a capacity that goes on with records that would vote if they were read"""
    rec = slab(n + 70, seed=n)
    p = PR.xyz(rec)
    p[n:, 1], p[n:, 2] = f32(0.6), f32(0.8)                       # on the plane
    sp = PR.spec(65, 0.02, 1.0, seed=n)
    planes, best, sums, marks = check(inst, sp, rec, f"n = {n}", n=n)
    assert not marks[n:].any() and planes["votes"].max() <= n
    if n < 3:
        assert planes.tobytes() == bytes(32 * 65) and PR.is_void(best) and not sums.any() and not marks.any()
    elif n == 3:
        assert set(planes["votes"].tolist()) == {0, 3} and sums[9] == 3
    else:
        assert planes["votes"].max() > n // 3
    fit(inst, PR.spec(65, 0.02, 1.0, seed=n, iterations=3), rec, f"fit, n = {n}", n=n)


def test_one_record_more_than_a_lap_of_each_grid(inst):
    rec = slab(VOTE_LAP + 1, seed=2)
    assert LAP + 1 < VOTE_LAP and len(rec) > 100000
    sp = PR.spec(3, 0.01, 1.0, seed=12)
    planes, best, sums, marks = check(inst, sp, rec, "a lap of the vote and one")
    assert planes["votes"].max() > 1000
    planes2, _, sums2, marks2 = check(inst, sp, rec, "a lap of the sums and one", n=LAP + 1)
    assert sums2[9] > 100 and marks2[:LAP + 1].any() and not marks2[LAP + 1:].any()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1024])
def test_every_number_of_candidates(inst, k):
    _, _, rec, _ = planted_scene()
    rec = rec[:601]
    planes, best, _, _ = check(inst, planted_spec(hypotheses=k, seed=k), rec, f"K = {k}")
    assert k == 1 or (not PR.is_void(best) and best["votes"] > 100)


def test_labels_take_records_out_and_the_call_writes_only_unlabelled_inliers(inst):
    _, _, rec, _ = planted_scene()
    labels = (np.arange(len(rec)) % 3 == 0).astype(np.uint8) * 77
    planes, best, sums, marks = check(inst, planted_spec(), rec, "labelled", labels=labels, value=200)
    free = check(inst, planted_spec(), rec, "unlabelled")
    assert best["votes"] < free[1]["votes"] and np.array_equal(marks == 77, labels == 77) and (marks == 200).sum() == best["votes"]


def test_non_finite_and_denormal_coordinates(inst):
    rec = edge_records()
    planes, best, sums, marks = check(inst, PR.spec(64, 0.01, 0.5, seed=9), rec, "edge records")
    assert 3 <= sum(not PR.is_void(p) for p in planes) < 64 and best["votes"] > 20
    bad = ~np.isfinite(PR.xyz(rec)).all(axis=1)
    assert bad.sum() == 5 and not marks[bad].any()
    # huge finite coordinates: products overflow, s is not finite, nothing votes and nothing faults
    huge = PR.records_of(np.random.default_rng(4).uniform(-3e38, 3e38, (300, 3)))
    check(inst, PR.spec(64, 1e30, 1e38, seed=1), huge, "huge records")


def test_a_collinear_list_has_no_plane_and_a_coplanar_one_ties_at_the_smallest_k(inst):
    line = collinear_records()
    planes, best, sums, marks = check(inst, PR.spec(64, 0.01, 1.0), line, "collinear")
    assert planes.tobytes() == bytes(32 * 64) and PR.is_void(best) and not sums.any() and not marks.any()
    plane, stats = fit(inst, PR.spec(64, 0.01, 1.0, iterations=3), line, "collinear fit")
    assert PR.is_void(plane) and stats["status"] == 1
    flat = coplanar_records()
    planes, best, sums, marks = check(inst, PR.spec(64, 0.01, 1.0, seed=2), flat, "coplanar")
    valid = [k for k in range(64) if not PR.is_void(planes[k])]
    assert len(valid) > 40 and all(planes["votes"][k] == len(flat) for k in valid) and best.tobytes() == planes[valid[0]].tobytes()
    assert sums[9] == len(flat) and (marks == 9).all()


def test_two_planted_planes_with_outliers(inst):
    _, _, rec, kind = planted_scene()
    n = len(rec)
    sp = planted_spec()
    floor, stats = fit(inst, sp, rec, "the first fit")
    assert stats["status"] == 0 and recovered(floor, FLOOR, stats["inliers"])
    # label the floor on the device with the fitted plane, then fit over the labels
    dev = Device(rec, 1, labels=np.zeros(n, np.uint8))
    d_plane = Shifted(32, floor, 16)
    dev.torch_sync()
    assert inst.plane_label(c_spec(sp), dev.rec.ptr, n, None, d_plane.ptr, 1, dev.labels.ptr) and inst.synchronize()
    labels = dev.labels.read("floor labels").copy()
    assert np.array_equal(labels, PR.label(sp, rec, n, floor, 1, np.zeros(n, np.uint8))) and (labels == 1).sum() == stats["inliers"]
    assert np.array_equal(labels == 1, PR.inliers(sp, rec, n, None, floor))
    got = inst.plane_fit(c_spec(sp), dev.rec.ptr, n, None, dev.labels.ptr, trace=True)
    want = PR.fit(sp, rec, n, labels)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
    assert want[1]["status"] == 0 and recovered(want[0], WALL, want[1]["inliers"])
    assert np.array_equal(dev.labels.read("labels after the second fit"), labels)      # the fit only reads them
    d_plane2 = Shifted(32, want[0], 16)
    assert inst.plane_label(c_spec(sp), dev.rec.ptr, n, None, d_plane2.ptr, 2, dev.labels.ptr) and inst.synchronize()
    both = dev.labels.read("both labels")
    assert np.array_equal(both == 1, labels == 1) and np.array_equal(both, PR.label(sp, rec, n, want[0], 2, labels)) and (both == 0).sum() < 0.15 * n
    assert d_plane.read("floor plane").tobytes() == floor.tobytes() and dev.rec.read("records").tobytes() == rec.tobytes()
    # the prior: along the smaller plane's normal, the first fit returns the smaller plane
    wall, st = fit(inst, planted_spec(axis=tuple(WALL[0]), min_cos=0.9), rec, "the fit with a prior")
    assert st["status"] == 0 and recovered(wall, WALL, st["inliers"]) and float(wall["normal"] @ WALL[0]) > 0.99


def test_sums_keep_eight_skip_the_next_float_and_round_halves_to_even(inst):
    sp, rec, plane = sums_edge_case()
    dev = Device(rec, 1)
    d_plane = Shifted(32, plane, 16)
    dev.torch_sync()
    assert inst.plane_sums(c_spec(sp), dev.rec.ptr, len(rec), None, None, d_plane.ptr, dev.sums.ptr) and inst.synchronize()
    got = dev.sums.read("edge sums").view(np.int64)
    assert got.tolist() == PR.sums(sp, rec, len(rec), None, plane).tolist() and got[9] == len(rec) - 2 and got[0] == (1 << 38) + (1 << 36) + 28


def test_the_lists_of_the_cloud_the_surface_points_and_the_mesh_queued_behind_their_calls(inst):
    """the small fused scene of the volume tests: each list's own call, then the vote, the best plane and the sums behind it with the
    list's count word and no synchronisation in between"""
    import torch
    from test_gpu_volume import Device as VolumeDevice, integrate
    v, s, poses, disp = noisy_scene()
    vdev = VolumeDevice(v)
    words = integrate(inst, vdev, s, poses, disp, label="noisy scene")
    cloud, offsets = CR.points(disp, s)
    surface = VR.crossings(words, v, 1)
    vertices = MR.mesh(words, v, 1)[0]
    sp = PR.spec(64, 0.03, 1.0, seed=6)
    cs = c_spec(sp)
    d_disp = torch.from_numpy(np.ascontiguousarray(disp)).cuda()
    for name, want, cap in (("cloud", cloud, s.frames * s.height * s.width), ("surface", surface, len(surface) + 5), ("mesh", vertices, len(vertices) + 5)):
        lst = Shifted(16 * cap, shift=16)
        counts = Shifted(16, shift=4)
        planes, best, sums = Shifted(32 * 64, shift=16), Shifted(32, shift=16), Shifted(80, shift=8)
        torch.cuda.synchronize()
        if name == "cloud":
            assert inst.cloud_points(c_source(s), d_disp.data_ptr(), None, None, lst.ptr, counts.ptr)
            count = counts.ptr + 4 * s.frames
        elif name == "surface":
            assert inst.volume_points(c_volume(v), vdev.voxels, 1, lst.ptr, cap, counts.ptr)
            count = counts.ptr
        else:
            tri = Shifted(16 * 4, shift=16)
            assert inst.volume_mesh(c_volume(v), vdev.voxels, 1, lst.ptr, cap, tri.ptr, 4, counts.ptr)
            count = counts.ptr
        assert inst.plane_votes(cs, lst.ptr, cap, count, None, planes.ptr) and inst.plane_best(planes.ptr, 64, best.ptr)
        assert inst.plane_sums(cs, lst.ptr, cap, count, None, best.ptr, sums.ptr) and inst.synchronize()
        n = len(want)
        rec = lst.read(name)[:16 * n]
        assert rec.tobytes() == want.tobytes() and n > 300, name
        w_planes = PR.votes(sp, rec, n)
        assert planes.read(name + " planes").tobytes() == w_planes.tobytes(), name
        assert best.read(name + " best").tobytes() == PR.best(w_planes).tobytes() and PR.best(w_planes)["votes"] > 50, name
        assert sums.read(name + " sums").view(np.int64).tolist() == PR.sums(sp, rec, n, None, PR.best(w_planes)).tolist(), name


def test_two_runs_give_the_same_bytes(inst):
    _, _, rec, _ = planted_scene()
    big = slab(VOTE_LAP // 4 + 77, seed=8)
    for name, r, sp in (("planted", rec, planted_spec()), ("slab", big, PR.spec(64, 0.01, 1.0, seed=3, iterations=4))):
        dev = Device(r, 64)
        runs = [dev.chain(inst, sp, name) for _ in range(2)]
        assert all(runs[0][i].tobytes() == runs[1][i].tobytes() for i in range(4)), name
        fits = [inst.plane_fit(c_spec(sp), dev.rec.ptr, len(r), None, None, trace=True) for _ in range(2)]
        assert fits[0][1] == fits[1][1] and all(fits[0][i].tobytes() == fits[1][i].tobytes() for i in (0, 2, 3)), name


def test_every_refusal_queues_nothing(inst):
    _, _, rec, _ = planted_scene()
    rec = rec[:256]
    dev = Device(rec, 8, n=256, labels=np.zeros(256, np.uint8))
    sp = planted_spec(hypotheses=8)
    cs = c_spec(sp)
    r, c, lb, pl, b, sm = dev.rec.ptr, dev.count.ptr, dev.labels.ptr, dev.planes.ptr, dev.best.ptr, dev.sums.ptr
    bad = c_spec(sp)
    bad.dist = -1.0
    dev.torch_sync()
    assert not inst.plane_votes(bad, r, 256, c, lb, pl) and not inst.plane_votes(cs, None, 256, c, lb, pl) and not inst.plane_votes(cs, r, 256, c, lb, None)
    assert not inst.plane_votes(cs, r + 8, 255, c, lb, pl) and not inst.plane_votes(cs, r, 256, c + 2, lb, pl) and not inst.plane_votes(cs, r, 256, c, lb, pl + 8)
    assert not inst.plane_votes(cs, r, (1 << 32) + 1, c, lb, pl) and not inst.plane_votes(cs, r, 256, c, lb, r + 32)
    assert not inst.plane_best(pl, 0, b) and not inst.plane_best(pl, 1025, b) and not inst.plane_best(pl, 8, pl + 32) and not inst.plane_best(pl, 8, b + 8)
    assert not inst.plane_sums(cs, r, (1 << 24) + 1, c, lb, b, sm) and not inst.plane_sums(cs, r, 256, c, lb, b, sm + 4) and not inst.plane_sums(cs, r, 256, c, lb, b, r + 16)
    assert not inst.plane_sums(cs, r, 256, c, lb, None, sm) and not inst.plane_sums(cs, r, 256, c, lb, b, b)
    assert not inst.plane_label(cs, r, 256, c, b, 0, lb) and not inst.plane_label(cs, r, 256, c, b, 256, lb) and not inst.plane_label(cs, r, 256, c, b, 1, None)
    assert not inst.plane_label(cs, r, 256, c, b, 1, r + 7) and not inst.plane_label(bad, r, 256, c, b, 1, lb)
    assert inst.plane_fit(bad, r, 256, c, lb) is None and inst.plane_fit(cs, r, (1 << 24) + 1, c, lb) is None and inst.plane_fit(cs, r + 4, 256, c, lb) is None
    assert inst.synchronize()
    for buf, name in ((dev.planes, "planes"), (dev.best, "best"), (dev.sums, "sums")):
        assert np.all(buf.read(name) == 0xA5), name
    dev.unchanged("refusals")
