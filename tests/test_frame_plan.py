"""The keyframe plan (pi-slam-fusion_amd/csrc/frame_plan.hpp -- the very code the library compiles: the cull's bounds, the need windows,
bitmaps and rectangles of the level launches) against models written from its rules, on the host, under AddressSanitizer and
UndefinedBehaviorSanitizer.  See tests/cpp/frame_plan_check.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_frame_plan_against_its_models(tmp_path):
    out = str(tmp_path)
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "plan", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "frame_plan_check")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "VIOLATION" not in text, text[-4000:]
    assert "frame plan ok" in text
    counts = {}
    for line in text.splitlines():
        if line.startswith(("plan:", "cull:")):
            w = line.split()[1:]
            counts.update({w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
    # a check that never exercised a branch must not pass: every count is non-trivial
    assert len(counts) == 30, counts
    for key, n in counts.items():
        assert n > 0, (key, counts)
    assert counts["bits_set"] > 1000 and counts["bits_clear"] > 100                 # (a) blocks needed and not needed
    assert counts["no_bitmap_wide"] > 0 and counts["no_bitmap_big"] > 0 and counts["overflow"] > 0      # canvases too wide, levels too large, > 64 cells
    assert counts["exact"] > 50 and counts["windows"] > 500 and counts["regions"] > 300       # (b), (c)
    assert counts["merge0"] > 10 and counts["mergeU"] > 10 and counts["must"] > 10000 and counts["empty_rect"] == 5 and counts["union"] > 50      # (d)
    assert counts["out"] > 1000 and counts["in"] > 1000 and counts["wmin_pos"] > 1000 and counts["frame_ok"] == 9 and counts["frame_bad"] == 1      # (e)
    assert counts["raised"] > 1000                                                   # (f)
    assert counts["tile_fresh"] > 1000 and counts["tile_whole"] > 100 and counts["tile_partial"] > 100 and counts["tile_pre"] > 100      # (g)
