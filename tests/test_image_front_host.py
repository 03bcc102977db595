"""The host side of the device image front end (no GPU): the library's LANCZOS tables are Pillow's.

sculpt_resample_lanczos_ksize / _coeffs against the Python restatement (tests/_lanczosref.py), those tables applied in numpy
against Image.resize(size, LANCZOS) bit for bit, the size arithmetic preprocess_image_device shares with frame_foreground, and
the coefficient code alone under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import _lanczosref as L
from conftest import ROOT

PAIRS = [(53, 320), (700, 320), (320, 701), (320, 97), (1500, 1024), (7, 2), (5, 3), (1, 4), (64, 64), (1, 1)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
def test_tables_equal_the_restatement(pair):
    from sculptmate_amd import ops

    ksize, bounds, kk = ops.lanczos_tables_host(*pair)
    rk, rb, rkk = L.tables(*pair)
    assert ksize == rk
    assert bounds.dtype == np.int32 and kk.dtype == np.int32 and kk.shape == (pair[1], ksize)
    assert np.array_equal(bounds, rb)
    assert np.array_equal(kk, rkk)
    # what the kernels rely on: every window lies inside the input and inside the table row
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all()
    assert (bounds[:, 0] + bounds[:, 1] <= pair[0]).all()


def test_tables_refuse_bad_arguments():
    import ctypes

    from sculptmate_amd import _lib, ops

    lib = _lib.lib
    assert lib.sculpt_resample_lanczos_ksize(0, 4) == 0 and lib.sculpt_resample_lanczos_ksize(4, -1) == 0
    assert lib.sculpt_resample_lanczos_ksize(1 << 20, 4) == 0
    with pytest.raises(ops.SculptError):
        ops.lanczos_tables_host(0, 4)
    b, k = np.zeros((4, 2), np.int32), np.zeros((4, 7), np.int32)
    assert lib.sculpt_resample_lanczos_coeffs(1, 4, 9, b.ctypes.data, k.ctypes.data) != 0 and "ksize" in _lib.last_error()
    assert lib.sculpt_resample_lanczos_coeffs(1, 4, 7, None, ctypes.c_void_p(k.ctypes.data)) != 0
    assert lib.sculpt_resample_lanczos_coeffs(1, 4, 7, b.ctypes.data, k.ctypes.data) == 0


@pytest.mark.parametrize("mode,shape,size", [
    ("RGB", (53, 37), (320, 320)), ("RGB", (513, 700), (320, 320)), ("RGB", (333, 333), (1024, 1024)),
    ("RGB", (700, 1024), (1024, 1024)), ("L", (320, 320), (701, 517)), ("L", (320, 320), (97, 1201)), ("L", (7, 5), (3, 2)),
], ids=lambda v: str(v).replace(" ", ""))
def test_library_tables_reproduce_pillow(mode, shape, size):
    """shape = (H, W) of the seeded input, size = Pillow's (width, height)."""
    from sculptmate_amd import ops

    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    a = rng.integers(0, 256, shape + ((3,) if mode == "RGB" else ()), dtype=np.uint8)
    want = np.array(Image.fromarray(a, mode=mode).resize(size, Image.LANCZOS))
    got = L.resize(a, size[1], size[0], table_fn=ops.lanczos_tables_host)
    assert np.array_equal(got, want)


def test_library_tables_reproduce_pillow_where_the_clamp_bites():
    from sculptmate_amd import ops

    a = (np.random.default_rng(5).integers(0, 2, (300, 200), dtype=np.uint8) * 255)
    want = np.array(Image.fromarray(a, mode="L").resize((320, 320), Image.LANCZOS))
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(L.resize(a, 320, 320, table_fn=ops.lanczos_tables_host), want)


@pytest.mark.parametrize("ratio", [0.75, 0.85])
def test_frame_layout_is_frame_foregrounds_arithmetic(ratio):
    """preprocessing.frame_layout gives the frame's side and the box's place in it exactly as the two paddings of
    frame_foreground do, odd remainders to the bottom and right."""
    from sculptmate_amd import preprocessing as P

    for h, w in [(1, 1), (10, 3), (3, 10), (7, 7), (101, 64), (64, 101), (0, 0), (0, 5)]:
        rgba = np.zeros((h + 5, w + 6, 4), np.uint8)
        rgba[2:2 + h + 1, 3:3 + w + 1, 3] = 200          # the box is [min, max): one row and one column are lost
        rgba[2:2 + h + 1, 3:3 + w + 1, 0] = np.arange(1, w + 2, dtype=np.uint8)[None, :]
        framed = P.frame_foreground(rgba, ratio)
        side, top, left = P.frame_layout(h, w, ratio)
        assert framed.shape == (side, side, 4)
        want = np.zeros_like(framed)
        want[top:top + h, left:left + w] = rgba[2:2 + h, 3:3 + w]
        assert np.array_equal(framed, want)


def _host_cxx():
    """A host C++ compiler: g++ or clang++ on the path, else the clang++ that ships with hipcc (the build needs that one anyway)."""
    from sculptmate_amd import build

    beside_hipcc = os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin", "clang++")
    for c in (shutil.which("g++"), shutil.which("clang++"), beside_hipcc):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler (g++, clang++ or hipcc's clang++) for the sanitizer run")


def test_coefficient_code_is_clean_under_asan_and_ubsan(tmp_path):
    """csrc/resample_coeffs.h is plain C++: a stand-alone driver fills the tables of every size pair above (1 -> 4 and 7 -> 2
    clamp the window at both ends) into exactly sized heap buffers under -fsanitize=address,undefined."""
    exe = str(tmp_path / "asan_resample_coeffs")
    src = os.path.join(ROOT, "tests", "native", "asan_resample_coeffs.cpp")
    c = subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", exe, src], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "asan_resample_coeffs ok" in p.stdout
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
