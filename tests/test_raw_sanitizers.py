"""The host raw-frame converter (csrc/raw_convert.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/san_raw_convert.cpp,
a stand-alone program, runs every format over the tiny shapes with heap buffers of exactly the bytes a descriptor promises and compares
with the pictures of tests/raw_model.py.  No GPU, no Python in the process under test."""
import os
import subprocess

import numpy as np

import raw_frames as rf
import raw_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_converter_under_address_and_ub_sanitizers(tmp_path):
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "raw_convert.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    d = tmp_path / "cases"; d.mkdir()
    cases = rf.cases()
    rng = np.random.default_rng(77)
    for i, (fmt, rows, cols) in enumerate(cases):
        views, _ = rm.random_planes(fmt, rows, cols, rng)
        (d / ("c%03d.txt" % i)).write_text("%d %d %d\n" % (fmt, rows, cols))
        for k, v in enumerate(views):
            (d / ("c%03d.p%d" % (i, k))).write_bytes(np.ascontiguousarray(v).tobytes())
        (d / ("c%03d.bgr" % i)).write_bytes(rm.to_bgr(fmt, views, rows, cols).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_raw_convert"), str(d), str(len(cases))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("cases ")][-1].split()
    assert int(line[1]) == len(cases) and int(line[3]) == 2 * len(cases) and int(line[5]) == 0
