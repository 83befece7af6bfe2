"""sgm_main --volume ... --volume-objects MINVOXELS[,CONN[,CLEARANCE]] on the stand-in device (tests/stub_device.c with the stand-in
launchers of the volume, the mesh, the plane and the components): the lines it prints and the vertex property it adds against the
restatements, with and without --plane, and that without the flag every output file and line is what it was; and, marked gpu, the real driver on a synthetic pair.
(The name sorts the file behind every existing one, for the reason tests/test_zz_components_cpu.py gives.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as CR
import mesh_ref as MR
import plane_ref as PR
import standin
from conftest import ROOT
from test_driver_mesh import FACE, WIDE, read_mesh_ply, spec_of
from test_driver_volume import PIN, want_of, write_pgm
from test_plane_cpu import driver_fit, plane_line

W, H = 70, 33


@pytest.fixture(scope="module")
def standin_driver(tmp_path_factory):
    csrc, t = standin.CSRC, os.path.join(ROOT, "tests")
    return standin.build(tmp_path_factory.mktemp("components_driver"), exe="sgm_main_standin", flags=("-ffp-contract=off",),
                         extra_sources=[os.path.join(csrc, "sgm_main.c"), os.path.join(csrc, "sgm_image_io.c")] +
                                       [os.path.join(t, "stub_%s.c" % n) for n in ("cloud", "plane", "volume", "raycast", "mesh", "color", "window",
                                                                                   "distance", "components")],
                         libs=("-lz",))


def read_object_ply(path, colours=False):
    """(xyz float32 [V][3], object uint32 [V], faces uint32 [F][3]) of a mesh PLY with the object property behind x y z (and colours)"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    nv, nf = (int([ln for ln in lines if ln.startswith("element " + name)][0].split()[-1]) for name in ("vertex", "face"))
    rgb = ["property uchar red", "property uchar green", "property uchar blue"] if colours else []
    assert lines[2:] == [f"element vertex {nv}", "property float x", "property float y", "property float z"] + rgb + \
        ["property uint object", f"element face {nf}", "property list uchar uint vertex_indices"]
    vertex = np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if colours else []) + [("object", "<u4")])
    assert len(body) == vertex.itemsize * nv + FACE.itemsize * nf
    v = np.frombuffer(body[:vertex.itemsize * nv], vertex)
    return v["xyz"], v["object"], np.frombuffer(body[vertex.itemsize * nv:], FACE)["v"]


def object_lines(v, objects, counts, min_voxels, connectivity, note=""):
    out = ["volume objects: %d of %d components have at least %d voxels (connectivity %d%s)" % (counts[0], counts[1], min_voxels, connectivity, note)]
    for i, o in enumerate(objects):
        lo, hi, c = CR.metric(v, o)
        out.append("volume object %d: %d voxels, box (%.9g, %.9g, %.9g) to (%.9g, %.9g, %.9g), centroid (%.9g, %.9g, %.9g)"
                   % ((i + 1, o["voxels"]) + tuple(lo) + tuple(hi) + tuple(c)))
    return out


def test_driver_on_the_stand_in_prints_the_objects_and_without_the_flag_what_it_wrote(standin_driver, tmp_path):
    """the stand-in's match leaves an all-zero map: with doffs 0.75 every pixel is kept, at Z = 40 / 0.75 -- one slab of occupied
    voxels behind a plane that faces the camera"""
    img = (np.arange(W * H, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(H, W)
    write_pgm(str(tmp_path / "l.pgm"), img)
    write_pgm(str(tmp_path / "r.pgm"), img)
    raw, ply, ply2, mesh, mesh2 = (str(tmp_path / n) for n in ("d.f32", "v.ply", "v2.ply", "m.ply", "m2.ply"))
    base = [standin_driver, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--max-disparity", "16", "--raw", raw,
            "--pinhole", ",".join(PIN)]
    vol = ["--volume", WIDE, "--volume-ply", ply]
    for extra, says in ((["--volume-objects", "3"], "--volume-objects needs --volume"),
                        (vol + ["--volume-objects", "x"], "--volume-objects wants MINVOXELS[,CONN[,CLEARANCE]]"),
                        (vol + ["--volume-objects", "0"], "--volume-objects wants MINVOXELS[,CONN[,CLEARANCE]]")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and says in out.stderr and "unknown option" not in out.stderr, (extra, out.stdout, out.stderr)
    plain = subprocess.run(base + vol + ["--volume-mesh", mesh, "--plane", "32,0.02,1"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "volume object" not in plain.stdout, (plain.stdout[-500:], plain.stderr[-500:])
    v = spec_of(WIDE)
    vox, pts = want_of(np.fromfile(raw, np.float32), W, H, WIDE)
    vert, tri = MR.mesh(vox, v, 1)
    said = lambda text: [ln for ln in text.splitlines() if not ln.startswith("volume object") and not re.search(r"\d ms\b", ln)]   # (times vary)

    # without --plane: the components of the occupied voxels, at 6 (the default) and at 26
    for arg, min_voxels, conn in (("1", 1, 6), ("5,26", 5, 26), ("100000,6", 100000, 6)):
        out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-mesh", mesh2, "--volume-objects", arg], capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
        labels, objects, counts = CR.call(vox, v, 1, connectivity=conn, min_voxels=min_voxels)
        assert counts[1] >= 1 and (counts[0] >= 1) == (min_voxels < 100000)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("volume object")]
        assert got == object_lines(v, objects, counts, min_voxels, conn), (got[:3], arg)
        # the other files are the same bytes, the mesh the same lists with one more property
        assert open(ply, "rb").read() == open(ply2, "rb").read()
        xyz, index, faces = read_object_ply(mesh2)
        xyz0, faces0 = read_mesh_ply(mesh)
        assert xyz.tobytes() == xyz0.tobytes() and faces.tobytes() == faces0.tobytes() and len(xyz) == len(vert) > 100
        assert np.array_equal(index, CR.component_of(labels, objects, counts[0], vert["id"], 8)) and (index != 0).all() == (counts[0] >= 1)
        assert said(out.stdout) == [ln for ln in said(plain.stdout) if not ln.startswith("plane")]

    # with --plane: the plane of the surface points, the one the driver prints afterwards, is excluded first.  It faces the camera
    # (normal (0, 0, -1)), so the slab lies behind it: a clearance of 0 leaves nothing, a negative one the voxels near the surface
    sp, (plane, stats, _, _) = driver_fit(PR.records_of(np.stack([pts["x"], pts["y"], pts["z"]], 1)), 32, 0.02, 1)
    assert stats["status"] == 0 and plane["normal"][2] == -1.0
    kept = []
    for clearance in ("0", "-4.5", "-100"):
        out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-mesh", mesh2, "--plane", "32,0.02,1", "--volume-objects",
                                     "1,26," + clearance], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
        labels, objects, counts = CR.call(vox, v, 1, connectivity=26, planes=[(plane["normal"], plane["anchor"])], clearance=[float(clearance)])
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("volume object")]
        assert got == object_lines(v, objects, counts, 1, 26, ", the plane excluded"), (got[:3], clearance)
        assert plane_line(plane, stats) in out.stdout.splitlines() and said(out.stdout) == said(plain.stdout)
        _, index, _ = read_object_ply(mesh2)
        assert np.array_equal(index, CR.component_of(labels, objects, counts[0], vert["id"], 8))
        kept.append(int((labels != 0).sum()))
    assert kept[0] == 0 < kept[1] < kept[2] == int(CR.member(vox, v, 1).sum())
    # a plane that is not found excludes nothing and is said so; with --volume-color the property follows the colours
    out = subprocess.run(base + ["--volume", WIDE, "--volume-ply", ply2, "--volume-mesh", mesh2, "--volume-color", "--plane", "16,0.01,5,1,0,0,0.9",
                                 "--volume-objects", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    labels, objects, counts = CR.call(vox, v, 1)
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("volume object")] == object_lines(v, objects, counts, 1, 6, ", no plane found")
    xyz, index, _ = read_object_ply(mesh2, colours=True)
    assert xyz.tobytes() == read_mesh_ply(mesh)[0].tobytes() and np.array_equal(index, CR.component_of(labels, objects, counts[0], vert["id"], 8))
    # a connectivity the library refuses fails the run
    out = subprocess.run(base + vol + ["--volume-objects", "1,18"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "sgm_mi355x: sgm_volume_components: a connectivity of 18" in out.stderr


@pytest.mark.gpu
def test_driver_on_the_device_prints_the_objects_of_its_own_map(tmp_path):
    """the real driver on a synthetic pair: the lines and the vertex property against the restatements on the map it wrote, with
    the plane it fitted excluded, and without the flag the same files"""
    from test_driver_volume import EXE
    import soc_project_stereo_matching_amd as S
    assert os.path.exists(EXE)
    w, h = 203, 77
    left, right = S.synth_pair(w, h, 64, 0x4F18)
    write_pgm(str(tmp_path / "l.pgm"), left)
    write_pgm(str(tmp_path / "r.pgm"), right)
    pin = ("100.0", "100.0", "101.0", "38.0", "0.5", "0.25")      # fb = 50: disparities 4..64 are depths 0.8..12
    volume = "64,24,40,0.05,-1.6,-0.6,0.5,0.2"
    raw, ply, mesh, ply2, mesh2 = (str(tmp_path / n) for n in ("d.f32", "v.ply", "m.ply", "v2.ply", "m2.ply"))
    base = [EXE, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "d.pgm"), "--raw", raw, "--pinhole", ",".join(pin),
            "--cloud-z-max", "8", "--volume", volume, "--plane", "64,0.05,3"]
    plain = subprocess.run(base + ["--volume-ply", ply, "--volume-mesh", mesh], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "volume object" not in plain.stdout, (plain.stdout[-500:], plain.stderr[-500:])
    out = subprocess.run(base + ["--volume-ply", ply2, "--volume-mesh", mesh2, "--volume-objects", "4,26,-0.1"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-500:])
    v = spec_of(volume)
    vox, pts = want_of(np.fromfile(raw, np.float32), w, h, volume, pin, z_max=8.0)
    sp, (plane, stats, _, _) = driver_fit(PR.records_of(np.stack([pts["x"], pts["y"], pts["z"]], 1)), 64, 0.05, 3)
    assert stats["status"] == 0 and plane_line(plane, stats) in out.stdout.splitlines()
    labels, objects, counts = CR.call(vox, v, 1, connectivity=26, min_voxels=4, planes=[(plane["normal"], plane["anchor"])], clearance=[-0.1])
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("volume object")]
    assert counts[0] >= 1 and got == object_lines(v, objects, counts, 4, 26, ", the plane excluded"), (got[:3], counts)
    vert, _ = MR.mesh(vox, v, 1)
    xyz, index, faces = read_object_ply(mesh2)
    xyz0, faces0 = read_mesh_ply(mesh)
    assert xyz.tobytes() == xyz0.tobytes() and faces.tobytes() == faces0.tobytes() and open(ply, "rb").read() == open(ply2, "rb").read()
    assert np.array_equal(index, CR.component_of(labels, objects, counts[0], vert["id"], 8)) and index.any()
    said = lambda text: [ln for ln in text.splitlines() if not ln.startswith("volume object") and not re.search(r"\d ms\b", ln)]
    assert said(out.stdout) == said(plain.stdout)
