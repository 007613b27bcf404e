"""The scalar encoder of the PNG of save_png (csrc/png_encode.hpp), its CRC / Adler functions and the host writer of single-band maps under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/san_png.cpp, a stand-alone program, runs them over the shapes and masks of
tests/png_model.py with heap buffers of exactly the promised bytes and an output block of exactly the bound, and compares with the files
of the model written here.  No GPU, no Python in the process under test."""
import os
import subprocess

import numpy as np

import png_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))


def test_encoder_checksums_and_writer_under_address_and_ub_sanitizers(tmp_path):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "png.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    d = tmp_path / "cases"; d.mkdir()
    cases = pm.cases()
    for i, (name, bgr, mask) in enumerate(cases):
        (d / ("c%03d.txt" % i)).write_text("%d %d %d\n" % (bgr.shape[0], bgr.shape[1], mask is not None))
        (d / ("c%03d.bgr" % i)).write_bytes(np.ascontiguousarray(bgr).tobytes())
        (d / ("c%03d.msk" % i)).write_bytes((mask if mask is not None else np.zeros(bgr.shape[:2], np.uint8)).tobytes())
        (d / ("c%03d.png" % i)).write_bytes(pm.encode(bgr, mask))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_png"), str(d), str(len(cases))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("cases ")][-1].split()
    assert int(line[1]) == len(cases) and int(line[3]) == 2 * len(cases) and int(line[5]) == 2 * len(cases) and int(line[7]) == 6 * len(cases) and int(line[9]) == 0
