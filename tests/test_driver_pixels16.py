"""The command-line driver with images of more than 8 bits per sample (no GPU): sgm_load_gray16 round-trips 16-bit PGM and PNG,
sgm_main --bits 0 / 12 pick the bits and reach SGM_SetPixelBits, a 16-bit file with the default --bits 8 fails with a message, and
the 16-bit decoders survive damaged files under AddressSanitizer / UBSan.  The match itself runs on the stand-in device (tests/
stub_device.c + tests/stub_pixels16.c): what is checked is what the driver loads, says and asks of the library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import standin
from conftest import ROOT

EXE = os.path.join(ROOT, "soc_project_stereo_matching_amd", "sgm_main")
CSRC = os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def standin_exe(tmp_path_factory):
    """sgm_main linked with the C host and the stand-in device, under ASan + UBSan: a program of its own"""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    return standin.build(tmp_path_factory.mktemp("main16"), sanitize=True, exe="sgm_main_p16", libs=("-lz",),
                         extra_sources=[os.path.join(CSRC, "sgm_main.c"), os.path.join(CSRC, "sgm_image_io.c"),
                                        os.path.join(ROOT, "tests", "stub_pixels16.c")])


def env():
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99")
    e.pop("LD_PRELOAD", None)
    return e


def write_pgm16(path, img, maxval):
    h, w = img.shape
    with open(path, "wb") as f:
        f.write(b"P5\n# a comment\n%d %d\n%d\n" % (w, h, maxval))
        f.write(img.astype(">u2").tobytes())


def read_pgm16(path):
    data = open(path, "rb").read()
    head, w, h, maxval = data.split(None, 4)[:4]
    assert head == b"P5" and int(maxval) == 65535
    body = data[len(data) - 2 * int(w) * int(h):]
    return np.frombuffer(body, ">u2").reshape(int(h), int(w)).astype(np.uint16)


def sample(w=53, h=37, top=65536, seed=1):
    img = np.random.RandomState(seed).randint(0, top, (h, w)).astype(np.uint16)
    step = top // 16
    img[:, :20] = (img[:, :20] // step) * step                  # flat areas so every PNG filter type gets used
    return img


def test_sgm_load_gray16_round_trips_pgm_and_png(exe, tmp_path):
    from PIL import Image
    img = sample()
    png, pgm, pgm12 = (str(tmp_path / n) for n in ("deep.png", "deep.pgm", "twelve.pgm"))
    Image.fromarray(img).save(png)
    assert Image.open(png).mode.startswith("I;16")
    write_pgm16(pgm, img, 65535)
    img12 = sample(top=4096, seed=2)
    write_pgm16(pgm12, img12, 4095)
    for src, want, maxval in ((png, img, 65535), (pgm, img, 65535), (pgm12, img12, 4095)):
        dst = str(tmp_path / "out.pgm")
        out = subprocess.run([exe, "--convert16", src, dst], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert f"maxval = {maxval}" in out.stdout and f"w = {want.shape[1]}, h = {want.shape[0]}" in out.stdout
        assert np.array_equal(read_pgm16(dst), want), src
    # an 8-bit file is widened unshifted
    g8 = (img >> 8).astype(np.uint8)
    small = str(tmp_path / "small.png")
    Image.fromarray(g8).save(small)
    out = subprocess.run([exe, "--convert16", small, str(tmp_path / "out8.pgm")], capture_output=True, text=True)
    assert out.returncode == 0 and "maxval = 255" in out.stdout
    assert np.array_equal(read_pgm16(str(tmp_path / "out8.pgm")), g8.astype(np.uint16))
    # what it cannot read: a maxval beyond 65535, a truncated body
    bad = str(tmp_path / "bad.pgm")
    open(bad, "wb").write(b"P5\n4 4\n70000\n" + bytes(32))
    assert subprocess.call([exe, "--convert16", bad, str(tmp_path / "o.pgm")], stderr=subprocess.DEVNULL) != 0
    open(bad, "wb").write(b"P5\n4 4\n4095\n" + bytes(31))
    assert subprocess.call([exe, "--convert16", bad, str(tmp_path / "o.pgm")], stderr=subprocess.DEVNULL) != 0


def test_a_16_bit_file_with_8_bits_fails_with_a_message(exe, tmp_path):
    from PIL import Image
    img = sample(40, 24)
    png, pgm = str(tmp_path / "deep.png"), str(tmp_path / "deep.pgm")
    Image.fromarray(img).save(png)
    write_pgm16(pgm, img, 4095)
    for src in (png, pgm):
        for extra in ([], ["--bits", "8"]):
            out = subprocess.run([exe, src, src, str(tmp_path / "o.png")] + extra, capture_output=True, text=True)
            assert out.returncode != 0
            assert "unsupported" in out.stderr and "Failed to load images" in out.stdout, (src, out.stderr, out.stdout)
    for bad in (["--bits", "7"], ["--bits", "17"], ["--bits"]):
        out = subprocess.run([exe, pgm, pgm, str(tmp_path / "o.png")] + bad, capture_output=True, text=True)
        assert out.returncode == 2, (bad, out.stderr)


def test_bits_0_and_12_reach_the_library(standin_exe, tmp_path):
    from PIL import Image
    w, h = 40, 24
    l12, r12 = sample(w, h, 4096, 3), sample(w, h, 4096, 4)
    l16 = sample(w, h, 65536, 5)
    l8 = (l12 >> 4).astype(np.uint8)
    files = {n: str(tmp_path / n) for n in ("l12.pgm", "r12.pgm", "l16.png", "l8.png")}
    write_pgm16(files["l12.pgm"], l12, 4095)
    write_pgm16(files["r12.pgm"], r12, 4095)
    Image.fromarray(l16).save(files["l16.png"])
    Image.fromarray(l8).save(files["l8.png"])
    out_png = str(tmp_path / "o.png")

    def run(left, right, *extra):
        out = subprocess.run([standin_exe, files[left], files[right], out_png, "--max-disparity", "16", *extra], capture_output=True,
                             text=True, env=env(), timeout=60)
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-1500:]
        return out

    out = run("l12.pgm", "r12.pgm", "--bits", "0")
    assert out.returncode == 0 and "maxval 4095, 12 bits per sample" in out.stdout, (out.stdout, out.stderr)
    out = run("l12.pgm", "r12.pgm", "--bits", "12")
    assert out.returncode == 0 and "12 bits per sample" in out.stdout
    out = run("l12.pgm", "l16.png", "--bits", "0")                  # the deeper file decides
    assert out.returncode == 0 and "maxval 65535, 16 bits per sample" in out.stdout
    out = run("l16.png", "l16.png", "--bits", "10")                 # allowed: samples beyond 10 bits saturate g8, and the driver says so
    assert out.returncode == 0 and "saturate" in out.stdout
    out = run("l8.png", "l8.png", "--bits", "0")                    # 8-bit files: the plain path
    assert out.returncode == 0 and "maxval 255, 8 bits per sample" in out.stdout
    out = run("l8.png", "l12.pgm", "--bits", "12")                  # an 8-bit file is widened unshifted beside a 12-bit one
    assert out.returncode == 0 and "12 bits per sample" in out.stdout
    out = run("l12.pgm", "r12.pgm")                                 # default --bits 8
    assert out.returncode != 0 and "unsupported" in out.stderr


def test_16_bit_decoders_are_asan_clean_on_damaged_files(standin_exe, tmp_path):
    from PIL import Image
    rng = np.random.RandomState(9)
    img = sample(31, 23)
    good = {"a.png": None, "b.pgm": None}
    Image.fromarray(img).save(str(tmp_path / "a.png"))
    write_pgm16(str(tmp_path / "b.pgm"), img, 65535)
    n_cases = 0
    for name in good:
        data = open(str(tmp_path / name), "rb").read()
        variants = [data] + [data[:k] for k in (0, 1, 8, 20, 33, len(data) // 2, len(data) - 5, len(data) - 1)]
        for _ in range(30):
            b = bytearray(data)
            for _ in range(rng.randint(1, 4)):
                b[rng.randint(0, len(b))] ^= 1 << rng.randint(0, 8)
            variants.append(bytes(b))
        for k, v in enumerate(variants):
            p = str(tmp_path / f"v{k}_{name}")
            open(p, "wb").write(v)
            out = subprocess.run([standin_exe, "--convert16", p, str(tmp_path / "out.pgm")], capture_output=True, text=True, env=env(),
                                 timeout=60)
            assert out.returncode in (0, 1), (name, k, out.returncode, out.stderr[-1500:])
            assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (name, k, out.stderr[-1500:])
            n_cases += 1
    assert n_cases == 2 * 39
