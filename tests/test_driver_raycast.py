"""sgm_main --volume ... --volume-view ZMIN,ZMAX,STEP[,MINWEIGHT] --volume-depth OUT.f32 --volume-normals OUT.f32: the volume the
frame was fused into rendered back into the frame's own camera.  Flag handling runs on the product's driver anywhere; the run itself
is followed on the stand-in device (the driver built with csrc/sgm_host.c, tests/stub_device.c, tests/stub_volume.c and
tests/stub_raycast.c, which compute for real)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as RR
import standin
import volume_ref as VR
from conftest import ROOT
from test_driver_volume import EXE, PIN, VOLUME, want_of, write_pgm
from test_raycast_cpu import same_maps

VIEW = "40.0,66.0,2.0"
WIDE = "36,18,8,3.0,-54.0,-27.0,41.5,6.0"                       # the whole image at the depth of the stand-in's map, 40 / 0.75


def test_usage_errors_are_told_apart(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    pin = ",".join(PIN)
    full = ["--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin]
    for extra, says in ((["--volume-view", VIEW, "--volume-depth", "d.f32"], "need --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC"),
                        (["--volume-depth", "d.f32"], "need --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC"),
                        (["--volume-normals", "n.f32", "--pinhole", pin], "need --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC"),
                        (full + ["--volume-view", VIEW], "come together"), (full + ["--volume-depth", "d.f32"], "come together"),
                        (full + ["--volume-normals", "n.f32"], "come together"),
                        (full + ["--volume-view", "1,2", "--volume-depth", "d.f32"], "--volume-view wants ZMIN,ZMAX,STEP[,MINWEIGHT]"),
                        (full + ["--volume-view", "a", "--volume-depth", "d.f32"], "--volume-view wants ZMIN,ZMAX,STEP[,MINWEIGHT]")):
        out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png")] + extra, capture_output=True, text=True)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    # the options are known: with everything given the run gets as far as loading the images
    out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png")] + full + ["--volume-view", VIEW + ",2", "--volume-depth", "d.f32",
                                                                                      "--volume-normals", "n.f32"], capture_output=True, text=True)
    assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("raycast_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"),
                                        os.path.join(ROOT, "tests", "stub_volume.c"), os.path.join(ROOT, "tests", "stub_raycast.c")], libs=("-lz",))


def test_driver_on_the_stand_in_renders_the_volume_of_its_map(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75; the maps the driver writes
    are the restatement's render of the volume that map gives, from the frame's own camera"""
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, depth, normals = (str(tmp_path / n) for n in ("d.f32", "v.ply", "z.f32", "n.f32"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN), "--volume", WIDE, "--volume-ply", ply]
    out = subprocess.run(base + ["--volume-view", VIEW, "--volume-depth", depth, "--volume-normals", normals], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vox, pts = want_of(np.fromfile(raw, np.float32), w, h, WIDE)
    f = [float(x) for x in WIDE.split(",")]
    v = VR.spec(int(f[0]), int(f[1]), int(f[2]), f[3], f[4:7], f[7], max_weight=65535)
    fx, fy, cx, cy = (float(x) for x in PIN[:4])
    vw = RR.view(w, h, fx, fy, cx, cy, *(float(x) for x in VIEW.split(",")))
    want_d, want_n, stats = RR.raycast(vox, v, vw, VR.pose()[None])
    assert stats["hits"] > 500 and stats["normals"] > 100
    assert f"volume view: {stats['hits']} of {w * h} pixels meet the surface" in out.stdout
    same_maps("depth", np.fromfile(depth, np.float32), want_d)
    same_maps("normals", np.fromfile(normals, np.float32), want_n)
    z = want_d[np.isfinite(want_d)].astype(np.float64)
    assert np.all(np.abs(z - 40.0 / 0.75) < 0.01)                 # the plane the map was
    # the depth alone, with a min_weight no voxel reaches: every pixel empty, no normals file
    os.remove(normals)
    out = subprocess.run(base + ["--volume-view", VIEW + ",2", "--volume-depth", depth], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"volume view: 0 of {w * h} pixels" in out.stdout and not os.path.exists(normals)
    assert np.all(np.fromfile(depth, np.float32).view(np.uint32) == 0x7FC00000)
    # a view out of range is reported, and nothing is written
    os.remove(depth)
    os.remove(ply)
    for view in ("66.0,40.0,2.0", "40.0,66.0,0", "40.0,66.0,2.0,0", "0,1000,0.001"):
        bad = subprocess.run(base + ["--volume-view", view, "--volume-depth", depth], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 1 and "volume unavailable" in bad.stdout and "sgm_volume_raycast: the view is outside its ranges" in bad.stderr, view
        assert not os.path.exists(depth) and not os.path.exists(ply)
