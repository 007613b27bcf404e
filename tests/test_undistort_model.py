"""Undistortion on the host: pf_undistort_table and pf_undistort_fit_camera against the numpy model (tests/undistort_model.py), the model
against data written by the reference's own Undistorter.h (tests/golden/undistort/*.npz: its remapX / remapY, a source frame and its
undistort() output, 64 x 48 each), against known answers where the reference is undefined, and a mutation check of those comparisons.

The golden cases look at the interior of the source only (0 uncovered entries, no tap past the last row or column), so the reference
is defined on every pixel and the whole image compares.  The three rules on which the library deviates from it (DESIGN.md
"Undistortion") have known answers instead: the identity remap returns the source, first column included (X == 0 is a valid entry),
and the half-pixel shift is the mean of four clamped neighbours, exact in float32."""
import os

import numpy as np
import pytest

import undistort_model as um

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort")
GOLDEN_CASES = ("ocv", "atan", "tangential", "atan_frac")

# exact in binary: the identity and the half-pixel shift come out without a rounding
PIN = [64, 48, 64, 64, 31.5, 23.5]
PIN_HALF = [64, 48, 64, 64, 31.0, 23.0]             # output pixel (x, y) looks at (x + 0.5, y + 0.5)
PIN_SMALL = [41, 23, 40, 40, 20.25, 11.0]           # another size
OCV = [64, 48, 50, 50, 31.3, 23.7, -0.28, 0.09, 0.001, -0.002, -0.01]
TANGENTIAL = [64, 48, 50, 50, 31.3, 23.7, -0.1, 0.02, 0.03, -0.025, 0.0]
ATAN = [64, 48, 50, 50, 31.3, 23.7, 0.9]
ATAN_FRAC = [64, 48, 0.625, 0.8125, 0.4890625, 0.49375, 0.9]
OUT = [64, 48, 60, 60, 31.5, 23.5]                  # sees the interior of the 50-px sources
OUT_WIDE = [64, 48, 30, 30, 31.5, 23.5]             # sees past them: uncovered entries
EXACT_CASES = {
    "identity": (PIN, PIN), "half_shift": (PIN, PIN_HALF), "other_size": (PIN, PIN_SMALL), "pinhole_wide": (PIN, OUT_WIDE),
    "ocv": (OCV, OUT), "tangential": (TANGENTIAL, OUT), "ocv_wide": (OCV, OUT_WIDE), "tangential_small": (TANGENTIAL, PIN_SMALL),
}
ATAN_CASES = {"atan": (ATAN, OUT), "atan_frac": (ATAN_FRAC, OUT), "atan_wide": (ATAN, OUT_WIDE), "atan_small": (ATAN, PIN_SMALL)}


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def ulps(a, b):
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---------------------------------------------------------------- the model against the reference's own output
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_model_reproduces_the_reference(name):
    g = golden(name)
    x, y, unc = um.table(g["camera_in"], g["camera_out"])
    assert unc == 0 and (g["x"] >= 0).all()
    assert np.array_equal(x, g["x"]) and np.array_equal(y, g["y"])
    # no tap of these cases is clamped: the reference is defined on every pixel
    assert g["x"].max() < g["src"].shape[1] - 1 and g["y"].max() < g["src"].shape[0] - 1 and g["x"].min() > 0
    assert np.array_equal(um.pixels(g["x"], g["y"], g["src"]), g["out"])


def test_golden_parameters_are_the_cases_named_here():
    for name, cam in (("ocv", OCV), ("atan", ATAN), ("tangential", TANGENTIAL), ("atan_frac", ATAN_FRAC)):
        g = golden(name)
        assert list(g["camera_in"]) == cam and list(g["camera_out"]) == OUT


# ---------------------------------------------------------------- known answers where the reference is undefined
def mean_of_four(src):
    """the half-pixel shift: coefficients 1/4 each, products and sums exact in float32, truncated; neighbours clamped"""
    s = src.astype(np.int32)
    r = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    d = np.concatenate([s[1:], s[-1:]], axis=0)
    dr = np.concatenate([d[:, 1:], d[:, -1:]], axis=1)
    return ((s + r + d + dr) // 4).astype(np.uint8)


def test_identity_returns_the_source():
    src = um.source_frame(48, 64, 1)
    x, y, unc = um.table(PIN, PIN)
    assert unc == 0 and (x[:, 0] == 0).all() and np.array_equal(x[0], np.arange(64, dtype=np.float32))
    assert np.array_equal(um.pixels(x, y, src), src)


def test_half_pixel_shift_is_the_mean_of_four_clamped_neighbours():
    src = um.source_frame(48, 64, 2)
    x, y, unc = um.table(PIN, PIN_HALF)
    assert unc == 0 and x[0, -1] == 63.5 and y[-1, 0] == 47.5
    assert np.array_equal(um.pixels(x, y, src), mean_of_four(src))


def test_uncovered_entries_are_black_and_alpha_is_ignored():
    src = um.source_frame(48, 64, 3, cn=4)
    x, y, unc = um.table(OCV, OUT_WIDE)
    assert 0 < unc < x.size and ((x < 0) == (y < 0)).all() and int((x < 0).sum()) == unc
    out = um.pixels(x, y, src)
    assert (out[x < 0] == 0).all() and out[x >= 0].any()
    assert np.array_equal(out, um.pixels(x, y, np.ascontiguousarray(src[:, :, :3])))


# ---------------------------------------------------------------- mutation check: the comparisons above notice
def test_comparisons_fail_for_a_rounding_model():
    for name in GOLDEN_CASES:
        g = golden(name)
        assert not np.array_equal(um.pixels(g["x"], g["y"], g["src"], truncate=False), g["out"]), name


def test_comparison_fails_without_the_clamp():
    src = um.source_frame(48, 64, 2)
    x, y, _ = um.table(PIN, PIN_HALF)
    got = um.pixels(x, y, src, clamp=False)
    want = mean_of_four(src)
    assert not np.array_equal(got, want)
    assert np.array_equal(got[:-1, :-1], want[:-1, :-1])            # ... in the last row and column, nowhere else
    assert (got[-1] != want[-1]).any() and (got[:, -1] != want[:, -1]).any()


def test_comparison_fails_for_the_reference_validity_slip():
    src = um.source_frame(48, 64, 1)
    src[:, 0] |= 1                                                   # no black pixel in the first column
    x, y, _ = um.table(PIN, PIN)
    got = um.pixels(x, y, src, valid_rule="gt0")
    assert not np.array_equal(got, src)
    assert (got[:, 0] == 0).all() and np.array_equal(got[:, 1:], src[:, 1:])
    assert np.array_equal(um.pixels(x, y, src), src)


# ---------------------------------------------------------------- the library's table against the model
@pytest.mark.parametrize("name", sorted(EXACT_CASES))
def test_library_table_equals_the_model(pf, name):
    cam_in, cam_out = EXACT_CASES[name]
    x, y, unc = um.table(cam_in, cam_out)
    got = pf.undistort_table(cam_in, cam_out)
    assert got is not None, pf.lib().pf_last_error()
    assert got[0].shape == (int(cam_out[1]), int(cam_out[0]))
    assert np.array_equal(got[0], x) and np.array_equal(got[1], y)
    assert got[2] == unc == int((x < 0).sum())
    if name.endswith("wide"):
        assert unc > 0
    if name in ("identity", "half_shift", "ocv", "tangential"):
        assert unc == 0


@pytest.mark.parametrize("name", sorted(ATAN_CASES))
def test_library_atan_table_within_one_ulp_of_the_model(pf, name):
    """libm's atan / tan and numpy's may differ in the last bit of the double, which can move the float by one ulp; the validity test is
    on the doubles, so an entry whose model coordinate lies within 1e-9 of a bound could flip -- the cases have no such entry"""
    cam_in, cam_out = ATAN_CASES[name]
    u, v, valid = um.coordinates(cam_in, cam_out)
    c = um.in_camera(cam_in)
    near = (np.abs(u) < 1e-9) | (np.abs(v) < 1e-9) | (np.abs(u - c["w"]) < 1e-9) | (np.abs(v - c["h"]) < 1e-9)
    assert int(near.sum()) == 0
    x, y, unc = um.table(cam_in, cam_out)
    gx, gy, gunc = pf.undistort_table(cam_in, cam_out)
    assert np.array_equal(gx < 0, ~valid) and np.array_equal(gy < 0, ~valid) and gunc == unc
    assert ulps(gx[valid], x[valid]).max() <= 1 and ulps(gy[valid], y[valid]).max() <= 1
    assert (gx[~valid] == -1).all() and (gy[~valid] == -1).all()
    if name.endswith("wide"):
        assert unc > 0


def test_table_refuses_what_is_no_camera(pf):
    for bad in ([64, 48, 50, 50, 31, 23, 0.1, 0.2], [64, 48], [0, 48, 50, 50, 31, 23], [64, 48, 0, 50, 31, 23], [64, 48, 50, float("nan"), 31, 23]):
        assert pf.undistort_table(bad, OUT) is None
        assert pf.fit_camera(bad, OUT) is None
    assert pf.undistort_table(OCV, [64, 48, 0, 60, 31.5, 23.5]) is None
    assert pf.undistort_table(OCV, [0, 48, 60, 60, 31.5, 23.5]) is None


# ---------------------------------------------------------------- fit_camera
def border_uncovered(cam_in, cam_out):
    x = um.table(cam_in, cam_out)[0]
    return int((x[0] < 0).sum() + (x[-1] < 0).sum() + (x[:, 0] < 0).sum() + (x[:, -1] < 0).sum())


@pytest.mark.parametrize("lens", ["ocv", "tangential", "atan"])
def test_fit_camera_is_the_smallest_scale_that_covers_the_border(pf, lens):
    cam_in = {"ocv": OCV, "tangential": TANGENTIAL, "atan": ATAN}[lens]
    want = OUT_WIDE
    assert border_uncovered(cam_in, want) > 0
    fit = pf.fit_camera(cam_in, want)
    assert fit is not None
    assert [fit[0], fit[1], fit[4], fit[5]] == [want[0], want[1], want[4], want[5]]
    k = int(round(fit[2] / want[2] * 4096))
    assert k > 4096 and fit[2] == (k / 4096) * want[2] and fit[3] == (k / 4096) * want[3]
    # the full table of the fitted camera has nothing uncovered, in the model's eyes and in the library's
    assert um.table(cam_in, fit)[2] == 0
    assert pf.undistort_table(cam_in, fit)[2] == 0
    less = list(want)
    less[2] = ((k - 1) / 4096) * want[2]; less[3] = ((k - 1) / 4096) * want[3]
    assert border_uncovered(cam_in, less) > 0


def test_dataset_config_carries_an_optional_input_camera(pf, tmp_path):
    """Map2D.InputCamera: 7 or 11 values, optional; Camera.Paraments keeps its six-value rule"""
    import importlib
    ds = importlib.import_module("pi_slam_fusion_amd.dataset")
    base = "Plane = 0 0 0 0 0 0 1\nCamera.Paraments = [64 48 60 60 31.5 23.5]\n"
    open(tmp_path / "trajectory.txt", "w").write("a 0 0 -100 0 0 0 1\n")
    open(tmp_path / "config.cfg", "w").write(base)
    assert ds.DroneMapDataset(str(tmp_path)).input_camera is None
    open(tmp_path / "config.cfg", "w").write(base + "Map2D.InputCamera = [%s]\n" % " ".join(repr(float(v)) for v in OCV))
    d = ds.DroneMapDataset(str(tmp_path))
    assert d.input_camera == OCV and d.camera == OUT
    open(tmp_path / "config.cfg", "w").write(base + "Map2D.InputCamera = [64 48 50 50 31.3 23.7 0.9]\n")
    assert ds.DroneMapDataset(str(tmp_path)).input_camera == ATAN
    open(tmp_path / "config.cfg", "w").write(base + "Map2D.InputCamera = [64 48 50 50 31.3 23.7]\n")
    with pytest.raises(ValueError):
        ds.DroneMapDataset(str(tmp_path))


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_plan_header_alone_under_sanitizers_says_the_same(pf, tmp_path):
    """csrc/undistort_plan.hpp in a stand-alone program built with ASan + UBSan, contraction off as in the library: the same tables,
    counts and fitted scales as the library gives, and hostile parameter vectors refused without a finding"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = str(tmp_path / "undistort_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + os.path.join(root, "pi-slam-fusion_amd", "csrc"), os.path.join(here, "cpp", "undistort_plan_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    good = [EXACT_CASES[k] for k in sorted(EXACT_CASES)] + [ATAN_CASES[k] for k in sorted(ATAN_CASES)]
    hostile = [([1e300, 48, 50, 50, 31, 23], OUT), ([64, 48, 50, 50, 31, 23, 1, 2], OUT), ([-5, 48, 50, 50, 31, 23], OUT), ([64, 48, 50, 0, 31, 23], OUT),
               (OCV, [64, 48, 0, 60, 31.5, 23.5]), (OCV, [1e12, 48, 60, 60, 31.5, 23.5]), ([64, 48, 50, 50, 31, 23, 1e308, 1e308, 1e308, 1e308, 1e308], OUT)]
    args = []
    for cam_in, cam_out in good + hostile:
        args += [str(len(cam_in))] + [repr(float(v)) for v in cam_in] + [repr(float(v)) for v in cam_out]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]
    lines = [[int(v) for v in l.split()] for l in text.splitlines() if l and l[0] in "01"]
    assert len(lines) == len(good) + len(hostile)
    for (cam_in, cam_out), got in zip(good, lines):
        x, y, unc = pf.undistort_table(cam_in, cam_out)
        fit = pf.fit_camera(cam_in, cam_out)
        k = 0 if fit is None else int(round(fit[2] / cam_out[2] * 4096))
        assert got == [1, unc, fnv(x), fnv(y), k], (cam_in, cam_out)
    for (cam_in, cam_out), got in zip(hostile[:-1], lines[len(good):]):
        assert got == [0, 0, 0, 0, 0] and pf.undistort_table(cam_in, cam_out) is None, (cam_in, cam_out)
    assert lines[-1][0] == 1 and lines[-1][1] == pf.undistort_table(*hostile[-1])[2]        # finite but absurd: a camera, mostly uncovered


def test_fit_camera_leaves_a_covered_camera_alone(pf):
    assert pf.fit_camera(OCV, OUT) == [float(v) for v in OUT]
    assert pf.Map2D.fit_camera(OCV, OUT) == [float(v) for v in OUT]
