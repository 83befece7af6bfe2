"""sgm_main --volume ... --volume-view ZMIN,ZMAX,STEP[,MINWEIGHT] --volume-track ITER,DISTMAX[,TX,TY,TZ]: the frame tracked against
the render of the volume it was fused into.  Flag handling runs on the product's driver anywhere; the run itself is followed on the
stand-in device (the driver built with csrc/sgm_host.c, tests/stub_device.c, tests/stub_volume.c, tests/stub_raycast.c and
tests/stub_track.c, which compute for real) and compared with the restatements, tolerance 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import raycast_ref as RR
import standin
import track_ref as TR
import volume_ref as VR
from conftest import ROOT
from test_driver_raycast import VIEW, WIDE
from test_driver_volume import EXE, PIN, VOLUME, want_of, write_pgm


def test_usage_errors_are_told_apart(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    pin = ",".join(PIN)
    full = ["--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin]
    needs = "--volume-track needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC and --volume-view ZMIN,ZMAX,STEP[,MINWEIGHT]"
    wants = "--volume-track wants ITER,DISTMAX[,TX,TY,TZ] with ITER >= 1"
    for extra, says in ((["--volume-track", "3,0.5"], needs), (full + ["--volume-track", "3,0.5"], needs),
                        (full + ["--volume-view", VIEW, "--volume-track", "3"], wants),
                        (full + ["--volume-view", VIEW, "--volume-track", "3,0.5,0.1"], wants),
                        (full + ["--volume-view", VIEW, "--volume-track", "3,0.5,0.1,0.2"], wants),
                        (full + ["--volume-view", VIEW, "--volume-track", "0,0.5"], wants),
                        (full + ["--volume-view", VIEW, "--volume-track", "a"], wants)):
        out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png")] + extra, capture_output=True, text=True)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    # the options are known, and the track alone is a reason for a view: the run gets as far as loading the images
    for track in ("3,0.5", "3,0.5,0.1,-0.1,0.2"):
        out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png")] + full + ["--volume-view", VIEW, "--volume-track", track],
                             capture_output=True, text=True)
        assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("track_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c")] +
                                       [os.path.join(ROOT, "tests", n) for n in ("stub_volume.c", "stub_raycast.c", "stub_track.c")], libs=("-lz",))


def test_driver_on_the_stand_in_tracks_the_frame_against_its_render(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 the frame is a plane at Z = 40 / 0.75, and so is the render of the
    volume it was fused into.  What the driver prints is what the restatements give for the same map: within the gate the solve sees
    one plane (status 2, the guess kept), beyond it nothing associates (status 1)"""
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, depth = (str(tmp_path / n) for n in ("d.f32", "v.ply", "z.f32"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN), "--volume", WIDE, "--volume-ply", ply, "--volume-view", VIEW]
    fx, fy, cx, cy, baseline, doffs = (float(x) for x in PIN)
    z_min, z_max, step = (float(x) for x in VIEW.split(","))
    f = [float(x) for x in WIDE.split(",")]
    v = VR.spec(int(f[0]), int(f[1]), int(f[2]), f[3], f[4:7], f[7], max_weight=65535)
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs)
    for track, t, status in (("3,0.5", (0.0, 0.0, 0.0), 2), ("2,0.5,0.1,-0.05,0.2", (0.1, -0.05, 0.2), 2), ("4,0.25,0,0,1.5", (0.0, 0.0, 1.5), 1)):
        out = subprocess.run(base + ["--volume-track", track], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
        disp = np.fromfile(raw, np.float32)
        vox, _ = want_of(disp, w, h, WIDE)
        want_d, want_n, stats = RR.raycast(vox, v, RR.view(w, h, fx, fy, cx, cy, z_min, z_max, step), VR.pose()[None])
        assert stats["normals"] > 100
        it, dist_max = int(track.split(",")[0]), float(track.split(",")[1])
        m = TR.model(w, h, fx, fy, cx, cy, dist_max, float(np.float32(0.5) * (np.float32(z_min) + np.float32(z_max))), iterations=it,
                     min_pixels=6, min_pivot=float(np.float32(1e-6)))
        guess = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1] + [float(np.float32(x)) for x in t], np.float64)
        poses, st, _, _ = TR.track(disp.reshape(1, h, w), s, m, guess[None], want_d, want_n)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("volume track:")]
        assert len(lines) == 3, out.stdout
        assert lines[0] == "volume track: frame 0 status %d, %d pixels, rms %.17g" % (st[0]["status"], st[0]["pixels"], st[0]["rms"])
        assert lines[1] == "volume track: pose" + "".join(" %.17g" % x for x in poses[0])
        assert lines[2] == "volume track: world pose" + "".join(" %.9g" % float(x) for x in TR.world_pose(VR.pose(), poses[0]))
        assert st[0]["status"] == status and (st[0]["pixels"] > 100) == (status == 2), st
        assert poses[0].tobytes() == guess.tobytes()               # a failed solve keeps the guess
        assert not os.path.exists(depth)                           # the track alone writes no map
    # with the maps written as well, they are the render's
    out = subprocess.run(base + ["--volume-track", "1,0.5", "--volume-depth", depth], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "volume track: frame 0 status 2" in out.stdout
    assert np.fromfile(depth, np.float32).view(np.uint32).tobytes() == want_d.view(np.uint32).tobytes()
    # a gate out of range is reported by the library, and the run fails
    bad = subprocess.run(base + ["--volume-track", "3,0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "sgm_track: the model is outside its ranges (dist_max finite and > 0)" in bad.stderr
