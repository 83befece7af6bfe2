"""sgm_main --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC --volume-ply OUT.ply (with --pinhole): the map fused into a TSDF volume with the
identity pose, the surface points as a PLY.  Flag handling runs on the product's driver anywhere; the run itself is followed on the
stand-in device (the driver built with csrc/sgm_host.c, tests/stub_device.c and tests/stub_volume.c, which computes for real) and,
with an MI355X, on the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import standin
import volume_ref as VR
from conftest import ROOT

EXE = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
PIN = ("40.0", "40.0", "34.5", "16.0", "1.0", "0.75")            # fb = 40: the stand-in's all-zero map is a plane at 40 / 0.75
VOLUME = "12,6,8,0.15,-0.9,-0.45,52.9,0.3"
PLY = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("element vertex")][0].split()[-1])
    assert len(body) == n * PLY.itemsize
    return np.frombuffer(body, PLY)


def want_of(disp, w, h, volume=VOLUME, pin=PIN, z_max=np.inf):
    f = [float(x) for x in volume.split(",")]
    v = VR.spec(int(f[0]), int(f[1]), int(f[2]), f[3], f[4:7], f[7], max_weight=65535)
    fx, fy, cx, cy, baseline, doffs = (float(x) for x in pin)
    s = CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs, z_max=z_max)
    vox, _ = VR.integrate(VR.empty(v), v, s, VR.pose()[None], disp.reshape(1, h, w))
    return vox, VR.crossings(vox, v, 1)


def test_usage_errors_are_told_apart(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    pin = ",".join(PIN)
    for extra, says in ((["--volume", VOLUME], "--volume and --volume-ply OUT.ply come together"),
                        (["--volume-ply", "v.ply"], "--volume and --volume-ply OUT.ply come together"),
                        (["--volume", VOLUME, "--volume-ply", "v.ply"], "--volume needs --pinhole"),
                        (["--volume", "12,6,8,0.15", "--volume-ply", "v.ply", "--pinhole", pin], "--volume wants NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC"),
                        (["--volume", "a,b", "--volume-ply", "v.ply", "--pinhole", pin], "--volume wants NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC"),
                        (["--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin, "--scale", "2"], "--scale does not combine with --volume")):
        out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png")] + extra, capture_output=True, text=True)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    # the options are known: with everything given the run gets as far as loading the images
    out = subprocess.run([EXE, "a.png", "b.png", str(tmp_path / "o.png"), "--volume", VOLUME, "--volume-ply", "v.ply", "--pinhole", pin],
                         capture_output=True, text=True)
    assert out.returncode != 2 and "Failed to load images" in out.stdout, (out.stdout, out.stderr)


@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    csrc = standin.CSRC
    return standin.build(tmp_path_factory.mktemp("volume_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c"),
                                        os.path.join(ROOT, "tests", "stub_volume.c")], libs=("-lz",))


def check_ply(ply, pts, img, w, h, pin=PIN):
    """the records are the restatement's points, coloured with the grey at the pixel they project to"""
    assert len(ply) == len(pts) and all(ply[n].tobytes() == pts[n].tobytes() for n in "xyz")
    fx, fy, cx, cy = (np.float32(x) for x in pin[:4])
    u = np.clip(np.floor(fx * (pts["x"] / pts["z"]) + cx + np.float32(0.5)), 0, w - 1).astype(int)
    v = np.clip(np.floor(fy * (pts["y"] / pts["z"]) + cy + np.float32(0.5)), 0, h - 1).astype(int)
    assert np.array_equal(ply["r"], img[v, u]) and np.array_equal(ply["r"], ply["g"]) and np.array_equal(ply["g"], ply["b"])


def test_driver_on_the_stand_in_writes_the_surface_of_its_map(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at one depth; what the driver writes is the
    restatement's surface of the volume that map gives"""
    w, h = 70, 33
    img = (np.arange(w * h, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(h, w)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply = str(tmp_path / "d.f32"), str(tmp_path / "v.ply")
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw]
    out = subprocess.run(base + ["--pinhole", ",".join(PIN), "--volume", VOLUME, "--volume-ply", ply], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vox, pts = want_of(np.fromfile(raw, np.float32), w, h)
    seen = int((VR.unpack(vox)[1] > 0).sum())
    assert len(pts) == 72 and seen > 200                          # the plane crosses every one of the 12 x 6 columns once
    assert f"volume: {seen} of {12 * 6 * 8} voxels seen, {len(pts)} surface points" in out.stdout
    check_ply(read_ply(ply), pts, img, w, h)
    # a volume the map never reaches: a PLY of no points
    out = subprocess.run(base + ["--pinhole", ",".join(PIN), "--volume", "4,4,4,0.1,-0.2,-0.2,1.0,0.05", "--volume-ply", ply], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "0 surface points" in out.stdout and len(read_ply(ply)) == 0
    # a spec or a pinhole out of range is reported, and nothing is written
    for extra in (["--pinhole", ",".join(PIN), "--volume", "0,6,8,0.15,-0.9,-0.45,52.9,0.3"], ["--pinhole", ",".join(PIN), "--volume", "12,6,8,0.15,-0.9,-0.45,52.9,0"],
                  ["--pinhole", "0,1,2,3,4,5", "--volume", VOLUME], ["--pinhole", ",".join(PIN), "--cloud-z-max", "-1", "--volume", VOLUME]):
        bad = subprocess.run(base + extra + ["--volume-ply", str(tmp_path / "bad.ply")], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 1 and "volume unavailable" in bad.stdout and not os.path.exists(str(tmp_path / "bad.ply")), extra


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
    raw, ply = str(tmp_path / "d.f32"), str(tmp_path / "v.ply")
    out = subprocess.run([EXE, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--raw", raw, "--pinhole", ",".join(pin),
                          "--cloud-z-max", "8", "--volume", volume, "--volume-ply", ply], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    vox, pts = want_of(np.fromfile(raw, np.float32), w, h, volume, pin, z_max=8.0)
    assert len(pts) > 200 and f"{len(pts)} surface points" in out.stdout
    check_ply(read_ply(ply), pts, left, w, h, pin)
