"""The scalar encoder of the lossless tile codec (csrc/deflate_rle.hpp) and the lossless host writer under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/cpp/san_deflate.cpp, a stand-alone program, runs them over the hostile tiles and tiny images with heap
buffers of exactly the promised bytes and an output block of exactly the bound, and compares with the streams of tests/deflate_model.py
written here.  No GPU, no Python in the process under test."""
import os
import subprocess

import numpy as np

import deflate_model as dm
import tiff_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))

IMAGES = [(1, 1), (7, 5), (2, 256), (256, 3), (40, 31), (255, 257), (300, 130)]


def test_encoder_and_writer_under_address_and_ub_sanitizers(tmp_path):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "deflate.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    d = tmp_path / "cases"; d.mkdir()
    tiles = dm.hostile_tiles()
    for i, k in enumerate(sorted(tiles)):
        (d / ("t%03d.bgr" % i)).write_bytes(np.ascontiguousarray(tiles[k]).tobytes())
        (d / ("t%03d.z" % i)).write_bytes(dm.encode_tile(tiles[k]))
    rng = np.random.default_rng(99)
    for i, (h, w) in enumerate(IMAGES):
        a = (np.cumsum(rng.integers(-3, 4, (h, w, 3)), axis=1) + 100).astype(np.uint8)
        m = (rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)
        bg, masked = (0, 255)[i % 2], i % 3 == 1
        (d / ("i%03d.txt" % i)).write_text("%d %d %d %d\n" % (h, w, bg, masked))
        (d / ("i%03d.bgr" % i)).write_bytes(a.tobytes())
        (d / ("i%03d.msk" % i)).write_bytes(m.tobytes())
        (d / ("i%03d.z" % i)).write_bytes(dm.encode_tile(tm.tiles_of(a)[0]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_deflate"), str(d), str(len(tiles)), str(len(IMAGES))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("tiles ")][-1].split()
    assert int(line[1]) == len(tiles) and int(line[3]) == 2 * len(tiles) and int(line[5]) == len(IMAGES) and int(line[7]) == 2 * len(IMAGES) and int(line[9]) == 0
