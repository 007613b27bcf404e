"""The cull's bounds with the pyramid's slack (pi-slam-fusion_amd/csrc/frame_plan.hpp: the cell itself, a Lipschitz slack, the inside
test over the pyramid's reach) against the weights of every pyramid level, computed on the host for seeded random tame homographies, under
AddressSanitizer and UndefinedBehaviorSanitizer.  See tests/cpp/cull_slack_check.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cull_bounds_hold_at_every_pyramid_level(tmp_path):
    out = str(tmp_path)
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "cull_slack.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "cull_slack_check")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    print(text[-2000:])
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "VIOLATION" not in text, text[-4000:]
    assert "cull slack ok" in text
    line = [ln for ln in text.splitlines() if ln.startswith("slack:")][0].split()[1:]
    n = {line[i]: int(line[i + 1]) for i in range(0, len(line), 2)}
    assert n["samples"] >= 30 and n["pixels"] > 10 ** 7 and n["tiles"] > 1000 and n["raise_tiles"] > 1000
    # not vacuous: a lower bound in at least a fifth of the cells; cells that only the new rule culls; bounds the floor rule keeps in
    assert 5 * n["lb_pos"] >= n["cells"], n
    assert n["new_only"] > 0 and n["both_out"] > 0 and n["out"] > 1000, n
    # the check can fail: without the slack the lower bound is violated somewhere in the same sample
    assert n["control_cells"] > 1000 and n["control_viol"] > 0, n
