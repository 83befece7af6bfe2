"""sgm_main --cloud OUT.ply --pinhole FX,FY,CX,CY,BASELINE,DOFFS [--cloud-z-max Z]: the valid pixels of the map as a binary PLY.
Flag handling runs anywhere (tests/test_cloud_cpu.py); the end-to-end run needs an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
from conftest import GOLDEN, ROOT, load_npz

EXE = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    head, _, body = raw.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    count = [int(t.split()[2]) for t in lines if t.startswith("element vertex")]
    props = [t for t in lines if t.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                     "property uchar blue"]
    assert len(count) == 1 and len(body) == count[0] * VERTEX.itemsize
    return np.frombuffer(body, VERTEX)


@pytest.mark.gpu
def test_cloud_is_read_cloud_of_the_same_pair_coloured_by_the_reference_image(tmp_path):
    import soc_project_stereo_matching_amd as S
    if not os.path.exists(EXE):
        pytest.skip("sgm_main not built (no hipcc here)")
    l, r = os.path.join(GOLDEN, "cone_im2.png"), os.path.join(GOLDEN, "cone_im6.png")
    z = load_npz("cone_inputs.npz")
    left, right = z["left"], z["right"]
    h, w = left.shape
    pin = ("1733.74", "1733.74", "225", "187.5", "536.62", "3.5")
    ply = str(tmp_path / "cone.ply")
    out = subprocess.run([EXE, l, r, str(tmp_path / "d.png"), "--cloud", ply, "--pinhole", ",".join(pin), "--cloud-z-max", "60000"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    got = read_ply(ply)
    fx, fy, cx, cy, baseline, doffs = (float(v) for v in pin)
    spec = S.cloud_spec(w, h, fx, fy, cx, cy, baseline, doffs, z_max=60000.0)
    i = S.SGMInstance(0)
    try:
        assert i.reset(w, h, S.default_option(64))               # the driver's options (main.c:48-65)
        disp = i.match(left, right)
        pts, off = i.read_cloud(spec)
    finally:
        i.close()
    assert off.tolist() == [0, got.size] and f"cloud: {got.size} points" in out.stdout
    assert 0.2 * w * h < got.size < np.isfinite(disp).sum()      # z_max cuts into the valid pixels
    for k in "xyz":
        assert np.array_equal(got[k].view(np.uint32), pts[k].view(np.uint32)), k
    grey = left[pts["pixel"] >> 16, pts["pixel"] & 0xFFFF]
    for k in ("red", "green", "blue"):
        assert np.array_equal(got[k], grey), k
    want = CR.points(disp, CR.spec(w, h, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, doffs=doffs, z_max=60000.0))
    assert pts.tobytes() == want[0].tobytes()
    # the right image as reference view: the colour is the right image's grey at the pixel
    ply_r = str(tmp_path / "cone_r.ply")
    subprocess.run([EXE, l, r, str(tmp_path / "d.png"), "--right-reference", "--cloud", ply_r, "--pinhole", ",".join(pin)], check=True,
                   capture_output=True, timeout=120)
    got_r = read_ply(ply_r)
    i = S.SGMInstance(0)
    try:
        i.set_reference_view(True)
        assert i.reset(w, h, S.default_option(64)) and i.match(left, right) is not None
        pts_r, _ = i.read_cloud(S.cloud_spec(w, h, fx, fy, cx, cy, baseline, doffs))
    finally:
        i.close()
    assert got_r.size == pts_r.size > 0.2 * w * h and np.array_equal(got_r["z"].view(np.uint32), pts_r["z"].view(np.uint32))
    assert np.array_equal(got_r["red"], right[pts_r["pixel"] >> 16, pts_r["pixel"] & 0xFFFF])
    assert not np.array_equal(got_r["red"], left[pts_r["pixel"] >> 16, pts_r["pixel"] & 0xFFFF])
    # raw images rectified ahead of the match: the colour is the rectified left image's
    import rectify_ref as RR
    from test_gpu_rectify import Rig, _calib_file
    calib = str(tmp_path / "calib.txt")
    _calib_file(calib, w, h)
    ply_c = str(tmp_path / "cone_c.ply")
    subprocess.run([EXE, l, r, str(tmp_path / "d.png"), "--rectify", calib, "--cloud", ply_c, "--pinhole", ",".join(pin)], check=True,
                   capture_output=True, timeout=120)
    got_c = read_ply(ply_c)
    rig = Rig(w, h)
    i = S.SGMInstance(0)
    try:
        assert rig.on(i) and i.reset(w, h, S.default_option(64)) and i.match(left, right) is not None
        pts_c, _ = i.read_cloud(S.cloud_spec(w, h, fx, fy, cx, cy, baseline, doffs))
    finally:
        i.close()
    rect_left = RR.remap(left, rig.lx, rig.ly)
    assert got_c.size == pts_c.size > 0 and np.array_equal(got_c["z"].view(np.uint32), pts_c["z"].view(np.uint32))
    assert np.array_equal(got_c["blue"], rect_left[pts_c["pixel"] >> 16, pts_c["pixel"] & 0xFFFF])
    assert not np.array_equal(got_c["blue"], left[pts_c["pixel"] >> 16, pts_c["pixel"] & 0xFFFF])
    # an intrinsic out of range is reported, not written
    bad = subprocess.run([EXE, l, r, str(tmp_path / "d.png"), "--cloud", str(tmp_path / "bad.ply"), "--pinhole", "0,1,2,3,4,5"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and not os.path.exists(str(tmp_path / "bad.ply"))
