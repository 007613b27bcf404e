"""The tie matrices of warp_ties.py, qualified on the CPU.

1. Every link of the warp's fp64 coordinate chain -- the reciprocal's last bit, 32/W against division, cvRound's tie rule, contraction
   and order of the row and column terms, the 64-wide block origin, W's precision -- changes rounded coordinates on these matrices
   when it is altered (>= 100 pixels summed over the list at scale 32, >= 10 at scale 1, on a 768 x 512 canvas), and none of them
   does on the generic control matrix, which stands for the homographies every other test feeds: that is the gap.  (W through fp32 is
   seen on the control too -- 278 pixels at scale 32, 16 at scale 1 -- and asserted so.)
2. The oracle's three warps against the model's restatements on every matrix, byte for byte on noise frames: the oracle's tie rule
   (lrint), its reciprocal and its block origin are what every GPU parity test is checked against.
Reference: OpenCV 2.4.9 imgwarp.cpp warpPerspectiveInvoker (SURVEY 8c rule 2): W = W ? 32./W : 0; X = cvRound(X0*W), round half even."""
import os
from fractions import Fraction

import numpy as np
import pytest

import warp_ties as wt
from helpers import workloads
from map_model import (_warp_coords, invert3x3, warp_linear_const_8u_inv, warp_linear_reflect_inv, warp_nearest_const_inv)

SCALES = (32.0, 1.0)
ROWS, COLS = wt.CANVAS


@pytest.fixture(scope="module")
def flips():
    """{matrix name: array (mutant, scale) of flipped pixels}, on invert3x3(M0): the matrix the kernels really get"""
    out = {}
    for name, M0 in wt.MATRICES:
        M = invert3x3(M0)
        base = wt.mutant_coords(M, ROWS, COLS, SCALES)
        ref = _warp_coords(M, ROWS, COLS, SCALES)           # the harness restates the model's routine: same coordinates unmutated
        assert all(np.array_equal(a, b) for p, q in zip(base, ref) for a, b in zip(p, q)), name
        out[name] = np.array([wt.flipped(base, wt.mutant_coords(M, ROWS, COLS, SCALES, m)) for m in wt.MUTANTS])
    return out


def test_fma_helper_is_correctly_rounded():
    """warp_ties.fma against exact rational arithmetic, on random operands and on sums that cancel to the last bits"""
    rng = np.random.RandomState(0)
    a = rng.uniform(-2, 2, 2000); b = rng.randint(-600, 600, 2000).astype(np.float64); c = rng.uniform(-900, 900, 2000)
    c[1000:] = -(a[1000:] * b[1000:]) * (1 + rng.randint(-4, 5, 1000) * 2.0 ** -52)
    got = wt.fma(a, b, c)
    for i in range(2000):
        assert got[i] == float(Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i])), i       # Fraction -> float rounds correctly


def test_exact_family_survives_the_inversion():
    for name in wt.EXACT:
        assert np.array_equal(invert3x3(wt.matrix(name)), wt.wanted(name)), name


def test_every_mutant_is_seen_on_the_tie_matrices(flips):
    total = sum(f for n, f in flips.items() if n != wt.CONTROL)
    print({m: total[i].tolist() for i, m in enumerate(wt.MUTANTS)})
    for i, m in enumerate(wt.MUTANTS):
        assert total[i, 0] >= 100, (m, "scale 32", int(total[i, 0]))
        assert total[i, 1] >= 10, (m, "scale 1", int(total[i, 1]))


def test_no_mutant_is_seen_on_the_control(flips):
    f = flips[wt.CONTROL]
    for i, m in enumerate(wt.MUTANTS):
        if m == "w_f32":
            assert f[i, 0] > 0, "the control no longer sees even W through fp32"
        else:
            assert f[i].tolist() == [0, 0], (m, f[i].tolist())


def test_ties_sit_on_the_border_decisions():
    """exact_shear_1 / exact_scale_2: the weight's nearest coordinate is exactly -1/2 and cols - 1/2 (rows - 1/2) on whole lines, so the
    tie rule decides the in-bounds flag; exact_shear_32: the 1/32-px coordinate ties at -1/64, cols - 1 - 1/64 and on the last two
    rows, so it decides between the fast taps and the reflected ones (warp_index.hpp tap_is_fast)."""
    srows, scols = wt.FRAME
    for name in ("exact_shear_1", "exact_scale_2"):      # a whole border line each: a frame row of 640 canvas pixels, a frame column of 240
        M = invert3x3(wt.matrix(name))
        (X, Y), = wt.mutant_coords(M, ROWS, COLS, (1.0,))
        (Xa, Ya), = wt.mutant_coords(M, ROWS, COLS, (1.0,), "half_away")
        inb = (X >= 0) & (X < scols) & (Y >= 0) & (Y < srows)
        inb_a = (Xa >= 0) & (Xa < scols) & (Ya >= 0) & (Ya < srows)
        assert (inb & ~inb_a).sum() >= 240 and (~inb & inb_a).sum() == 0, name        # -1/2 -> 0 under half-even alone
        (Xu, Yu), = wt.mutant_coords(M, ROWS, COLS, (1.0,), "rcp_dn")
        inb_u = (Xu >= 0) & (Xu < scols) & (Yu >= 0) & (Yu < srows)
        assert (~inb & inb_u).sum() >= 240, name                                       # cols - 1/2 -> cols - 1 when the product falls short
    M = invert3x3(wt.matrix("exact_shear_32"))
    (X, Y), = wt.mutant_coords(M, ROWS, COLS, (32.0,))
    (Xa, Ya), = wt.mutant_coords(M, ROWS, COLS, (32.0,), "half_away")

    def fast(X, Y):
        return ((X >> 5) >= 0) & ((X >> 5) < scols - 1) & ((Y >> 5) >= 0) & ((Y >> 5) < srows - 2)
    assert (fast(X, Y) != fast(Xa, Ya)).sum() >= 300
    # rows - 2 - 1/64 and rows - 1 - 1/64 are ties above an odd integer, which every tie rule sends up: there a product one ulp short decides
    (Xd, Yd), = wt.mutant_coords(M, ROWS, COLS, (32.0,), "rcp_dn")
    for r in (srows - 2, srows - 1):
        assert (((Y >> 5) == r) & ((Yd >> 5) == r - 1)).sum() >= 640, r


def test_the_hook_is_in_the_experiments_library_alone():
    """pf_debug_next_homography (what test_gpu_warp_ties.py injects its matrices with) is test infrastructure: not in the product
    library, not declared in include/pifusion.h"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = b"pf_debug_next_homography"
    assert name not in open(os.path.join(root, "pi-slam-fusion_amd", "libpifusion.so"), "rb").read()
    assert name in open(os.path.join(root, "pi-slam-fusion_amd", "libpifusion_exp.so"), "rb").read()
    assert name not in open(os.path.join(root, "include", "pifusion.h"), "rb").read()


@pytest.fixture(scope="module")
def frames():
    wl = workloads()
    srows, scols = wt.FRAME
    bgr = wl.noise_frame(srows, scols, 7)
    bgra = wl.splitmix64_bytes(77, srows * scols * 4).reshape(srows, scols, 4)
    wgt = (wl.splitmix64_bytes(78, srows * scols * 2).view(np.uint16).astype(np.float32) * np.float32(1 / 65536)).reshape(srows, scols)
    return bgr.astype(np.int16), bgr.astype(np.float32) * np.float32(1. / 255.), wgt, bgra


@pytest.mark.parametrize("name", wt.NAMES)
def test_oracle_ops_equal_the_model(orc, frames, name):
    """orc.warp_linear_reflect (16S, 32F), orc.warp_nearest_const and orc.warp_linear_const_8u against map_model's restatements: noise
    frames, so that a coordinate one 1/32 px off shows in the pixel."""
    s16, s32, wgt, bgra = frames
    M0 = wt.matrix(name)
    M = invert3x3(M0)
    xy32, xy1 = _warp_coords(M, ROWS, COLS, SCALES)
    assert np.array_equal(orc.warp_linear_reflect(s16, M0, ROWS, COLS), warp_linear_reflect_inv(s16, M, ROWS, COLS, False, xy32))
    assert np.array_equal(orc.warp_linear_reflect(s32, M0, ROWS, COLS), warp_linear_reflect_inv(s32, M, ROWS, COLS, True, xy32))
    assert np.array_equal(orc.warp_nearest_const(wgt, M0, ROWS, COLS)[:, :, 0], warp_nearest_const_inv(wgt, M, ROWS, COLS, xy1))
    assert np.array_equal(orc.warp_linear_const_8u(bgra, M0, ROWS, COLS), warp_linear_const_8u_inv(bgra, M, ROWS, COLS, xy32))


def test_a_flipped_coordinate_shows_in_the_ops(frames):
    """the comparison above is not blind: the model's warps fed the half-away coordinates of one tie matrix differ from the oracle"""
    s16, s32, wgt, bgra = frames
    M = invert3x3(wt.matrix("exact_shear_32"))
    xy32, xy1 = wt.mutant_coords(M, ROWS, COLS, SCALES, "half_away")
    ok32, ok1 = _warp_coords(M, ROWS, COLS, SCALES)
    assert not np.array_equal(warp_linear_reflect_inv(s16, M, ROWS, COLS, False, xy32), warp_linear_reflect_inv(s16, M, ROWS, COLS, False, ok32))
    assert not np.array_equal(warp_nearest_const_inv(wgt, M, ROWS, COLS, xy1), warp_nearest_const_inv(wgt, M, ROWS, COLS, ok1))
    assert not np.array_equal(warp_linear_const_8u_inv(bgra, M, ROWS, COLS, xy32), warp_linear_const_8u_inv(bgra, M, ROWS, COLS, ok32))
