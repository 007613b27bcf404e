"""The reduced-resolution views (pf_blend_tiles_level, pf_blend_changed_level, pf_save_to_memory_level) without a GPU: the model of
the views (level_view_model.py) against ModelMap at level 0 and against the meaning of a truncated collapse -- the Gaussian level k,
computed by pyrDown alone -- and the new symbols of the C ABI and members of the C++ face."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from level_view_model import collapse_from, lattice_model, model_blend_level, model_save_level
from map_model import create_laplace_pyr, pyr_down, to_8u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pf_blend_tiles_level", "pf_blend_changed_level", "pf_save_to_memory_level")


@pytest.mark.parametrize("force_float", [0, 1])
def test_level_0_of_the_model_is_the_model_map(orc, force_float):
    """k = 0 is Ele::blend / save() themselves: both blend paths, raw and 8U, and the mosaic with its origin, exactly"""
    _, _, _, m = lattice_model(force_float, 5)
    tiles = m.tiles()
    full = [t for t in tiles if all((t[0] + dx, t[1] + dy) in m.tiles_ for dx in (-1, 0, 1) for dy in (-1, 0, 1))]
    assert full and len(full) < len(tiles)
    for t in tiles:
        raw = model_blend_level(m, *t, 0)
        assert raw.dtype == m.dtype and np.array_equal(raw, m.blend_tile_raw(*t)), t
        assert np.array_equal(to_8u(raw), m.blend_tile(*t)), t
    assert model_blend_level(m, 10 ** 6, 0, 0) is None
    img, origin = model_save_level(m, 0)
    ref, ref_origin = m.save()
    assert origin == ref_origin and np.array_equal(img, ref)
    for k in range(1, m.L + 1):                                     # and the shapes above it
        assert model_blend_level(m, *full[0], k).shape == (256 >> k, 256 >> k, 3)
        assert model_save_level(m, k)[0].shape == (ref.shape[0] >> k, ref.shape[1] >> k, 3)


def test_truncated_collapse_is_the_gaussian_level_fp32():
    """Collapsing a Laplacian pyramid from the top down to level k gives the Gaussian level k -- here computed by pyrDown alone, which
    shares nothing with the collapse.  The identity is exact in real arithmetic (L_i = G_i - pyrUp(G_{i+1}) is added back to the same
    pyrUp); in fp32 every level adds one rounding of the subtraction and one of the addition, a few ulps of 1.0 over <= 5 levels."""
    rng = np.random.RandomState(5)
    img = rng.uniform(0, 1, (96, 160, 3)).astype(np.float32)
    lap = create_laplace_pyr(img, 5)
    g = img
    for k in range(6):
        got = collapse_from(lap, k)
        assert got.shape == g.shape and got.dtype == np.float32
        assert np.abs(got - g).max() <= 1e-5, k
        g = pyr_down(g)
    assert np.array_equal(collapse_from(lap, 5), lap[5])


def test_truncated_collapse_is_the_gaussian_level_int16():
    """The same for 16S.  The model's own maximum difference, measured here on the CPU: 0 at every level -- with 8-bit content
    neither the saturating subtraction of createLaplacePyr nor the saturating add of the restore saturates, so adding back the same
    pyrUp is exact.  The bound is that measurement plus nothing."""
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (96, 160, 3)).astype(np.int16)
    lap = create_laplace_pyr(img, 5)
    g = img
    for k in range(6):
        got = collapse_from(lap, k)
        assert got.dtype == np.int16 and np.array_equal(got, g), k
        g = pyr_down(g)


def test_level_symbols_are_declared_exported_and_null_safe(pf):
    header = open(os.path.join(ROOT, "include", "pifusion.h")).read()
    L = pf.lib()
    for s in SYMBOLS:
        assert "int     %s(pf_map* m" % s in header, s
        assert hasattr(L, s), s
    xy = (ctypes.c_int * 2)(0, 0)
    px = np.full(256 * 256 * 3, 0xA5, np.uint8)
    r, c, x0, y0 = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    assert L.pf_blend_tiles_level(None, xy, 1, 0, px.ctypes.data, None) == 0
    assert L.pf_blend_changed_level(None, 0, xy, px.ctypes.data, 1) == 0
    assert L.pf_save_to_memory_level(None, 0, px.ctypes.data, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0)) == 0
    assert (px == 0xA5).all() and (r.value, c.value, x0.value, y0.value) == (7, 7, 7, 7)


def test_cpp_face_level_members_compile():
    """the new members of include/pifusion/Map2D.h, called from tests/cpp/level_view_smoke.cpp: syntax and types, plain g++ -std=c++11"""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "level_view_smoke.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
