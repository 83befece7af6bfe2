"""sgm_main --volume ... --volume-mesh OUT.ply: the volume the frame was fused into as a triangle mesh (sgm_volume_mesh), a binary
little-endian PLY of vertices and faces.  Flag handling runs on the product's driver anywhere; the run itself is followed on the
stand-in device (the driver built with csrc/sgm_host.c, tests/stub_device.c, tests/stub_volume.c and tests/stub_mesh.c, which
compute for real) and, with an MI355X, on the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_ref as MR
import standin
import volume_ref as VR
from conftest import ROOT
from test_driver_volume import EXE, PIN, VOLUME, want_of, write_pgm

WIDE = "36,18,8,3.0,-54.0,-27.0,41.5,6.0"                       # the whole image at the depth of the stand-in's map, 40 / 0.75
FACE = np.dtype([("n", "u1"), ("v", "<u4", (3,))])


def read_mesh_ply(path):
    """(xyz float32 [V][3], faces uint32 [F][3]) of a PLY with exactly the two elements the driver writes"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv, nf = (int([ln for ln in lines if ln.startswith("element " + name)][0].split()[-1]) for name in ("vertex", "face"))
    assert lines[2:] == [f"element vertex {nv}", "property float x", "property float y", "property float z", f"element face {nf}",
                         "property list uchar uint vertex_indices"]
    assert len(body) == 12 * nv + FACE.itemsize * nf and FACE.itemsize == 13
    faces = np.frombuffer(body[12 * nv:], FACE)
    assert np.all(faces["n"] == 3)
    return np.frombuffer(body[:12 * nv], "<f4").reshape(nv, 3), faces["v"]


def spec_of(volume):
    f = [float(x) for x in volume.split(",")]
    return VR.spec(int(f[0]), int(f[1]), int(f[2]), f[3], f[4:7], f[7], max_weight=65535)


def check_mesh(path, vox, v, stdout):
    vert, tri = MR.mesh(vox, v, 1)
    xyz, faces = read_mesh_ply(path)
    assert f"volume mesh: {len(vert)} vertices, {len(tri)} triangles" in stdout
    assert xyz.tobytes() == np.stack([vert["x"], vert["y"], vert["z"]], axis=1).tobytes()
    assert faces.tobytes() == tri["v"].tobytes()
    return vert, tri


def test_usage_errors_are_told_apart(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    pin = ",".join(PIN)
    out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png"), "--volume-mesh", "m.ply", "--pinhole", pin], capture_output=True, text=True)
    assert out.returncode == 2 and "--volume-mesh needs --volume" in out.stderr and "unknown option" not in out.stderr
    out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png"), "--volume-mesh"], capture_output=True, text=True)
    assert out.returncode == 2
    # the option is known: with everything given the run gets as far as loading the images
    out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png"), "--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin,
                          "--volume-mesh", "m.ply"], capture_output=True, text=True)
    assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("mesh_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"),
                                        os.path.join(ROOT, "tests", "stub_volume.c"), os.path.join(ROOT, "tests", "stub_mesh.c")], libs=("-lz",))


def test_driver_on_the_stand_in_writes_the_mesh_of_its_map(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75; the PLY the driver writes
    holds the restatement's lists for the volume that map gives"""
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, mesh = (str(tmp_path / n) for n in ("d.f32", "v.ply", "m.ply"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN)]
    out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply, "--volume-mesh", mesh], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vox, pts = want_of(np.fromfile(raw, np.float32), w, h, WIDE)
    vert, tri = check_mesh(mesh, vox, spec_of(WIDE), out.stdout)
    assert len(tri) > 500 and len(pts) == int(((vert["id"] & 7) < 3).sum())
    z = vert["z"][tri["v"]].astype(np.float64)
    assert np.all(np.abs(z - 40.0 / 0.75) < 0.01)                 # the plane the map was
    # a volume the map never reaches: a PLY with no vertex and no face
    out = subprocess.run(base + ["--volume", "4,4,4,0.1,-0.2,-0.2,1.0,0.05", "--volume-ply", ply, "--volume-mesh", mesh], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "volume mesh: 0 vertices, 0 triangles" in out.stdout
    xyz, faces = read_mesh_ply(mesh)
    assert len(xyz) == 0 and len(faces) == 0


def test_driver_without_the_mesh_launchers_reports_it(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    exe = standin.build(tmp_path, exe="sgm_main_standin", flags=("-ffp-contract=off",),
                        extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"),
                                       os.path.join(ROOT, "tests", "stub_volume.c")], libs=("-lz",))
    img = np.zeros((33, 70), np.uint8)
    write_pgm(str(tmp_path / "l.pgm"), img)
    mesh = str(tmp_path / "m.ply")
    out = subprocess.run([exe, str(tmp_path / "l.pgm"), str(tmp_path / "l.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--pinhole",
                          ",".join(PIN), "--volume", WIDE, "--volume-ply", str(tmp_path / "v.ply"), "--volume-mesh", mesh],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "volume unavailable" in out.stdout and "the mesh is not part of this build" in out.stderr
    assert not os.path.exists(mesh)


@pytest.mark.gpu
def test_driver_on_the_device_equals_the_restatement_on_its_own_map(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    import soc_project_stereo_matching_amd as S
    w, h = 203, 77
    left, right = S.synth_pair(w, h, 64, 0x4F18)
    write_pgm(str(tmp_path / "l.pgm"), left)
    write_pgm(str(tmp_path / "r.pgm"), right)
    pin = ("100.0", "100.0", "101.0", "38.0", "0.5", "0.25")      # fb = 50: disparities 4..64 are depths 0.8..12
    volume = "64,24,40,0.05,-1.6,-0.6,0.5,0.2"
    raw, ply, mesh = (str(tmp_path / n) for n in ("d.f32", "v.ply", "m.ply"))
    out = subprocess.run([EXE, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--raw", raw, "--pinhole", ",".join(pin),
                          "--cloud-z-max", "8", "--volume", volume, "--volume-ply", ply, "--volume-mesh", mesh], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vox, _ = want_of(np.fromfile(raw, np.float32), w, h, volume, pin, z_max=8.0)
    vert, tri = check_mesh(mesh, vox, spec_of(volume), out.stdout)
    assert len(tri) > 300
