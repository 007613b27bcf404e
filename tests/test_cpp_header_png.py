"""Map2D::savePng of the header-only C++ face compiles against libpifusion.so with plain g++ and behaves: nothing to save on a box without
a device, an RGB and an RGBA file on a GPU (tests/cpp/header_png.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp):
    exe = os.path.join(tmp, "header_png")
    lib = os.path.join(ROOT, "pi-slam-fusion_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "header_png.cpp"), "-o", exe,
                           "-L" + lib, "-l:libpifusion.so", "-lpthread", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_save_png_compiles_and_fails_loudly_without_device(pf, tmp_path):
    r = subprocess.run([build(str(tmp_path)), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()


@pytest.mark.gpu
def test_save_png_writes_both_files_on_gpu(pf, tmp_path):
    r = subprocess.run([build(str(tmp_path)), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"png files written" in r.stdout, r.stdout.decode()
