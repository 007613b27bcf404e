"""tests/bgra.py's frames on the CPU: the alpha planes keep their distance from the colours on every hostile frame, the padded layouts
are what they say, and -- the point -- a map whose gather leaks alpha differs from the true one for EVERY kind of frame, "const" and
"white" included, so that the comparisons of tests/test_gpu_bgra.py can fail for each of them.  Two mutants of ModelMap: the gather
slipped by one byte (channels 1..3 of the BGRA frame), and the "hi" tap that lies in the frame's last column taken from that pixel's
alpha byte (the last 8-byte load of a row, where the border path shifts by 8 * cn)."""
import numpy as np
import pytest

import bgra
import map_model
from helpers import HOSTILE_KINDS, hostile_frame, workloads
from map_model import ModelMap
from test_gpu_model import BG, CAM, witnesses

ROWS, COLS = 480, 640


@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_alpha_is_apart_from_every_colour(kind):
    planes = []
    for k in range(4):
        bgr = hostile_frame(kind, ROWS, COLS, k)
        f = bgra.with_alpha(bgr, k)
        assert f.shape == (ROWS, COLS, 4) and f.dtype == np.uint8 and np.array_equal(f[:, :, :3], bgr)
        assert bgra.apart(f) >= bgra.ALPHA_GAP
        assert set(np.unique(f[:, :, 3])) <= set(bgra.ALPHA_CANDIDATES)
        planes.append(f[:, :, 3])
    if kind == "white":                                   # 255 is blocked: the orders that begin with 255 or 0 take 0, then 128, then 64
        y, x = np.mgrid[0:ROWS, 0:COLS]
        for k, p in enumerate(planes):
            assert np.array_equal(p, np.array([0, 0, 128, 64], np.uint8)[(x + y + k) % 4])
    assert all(not np.array_equal(planes[k], planes[k + 1]) for k in range(3))


def test_alpha_against_a_scalar_restatement():
    """with_alpha pixel by pixel in plain Python, on colours that block up to three candidates (one colour value blocks at most one:
    255 / 0 / 128 / 64 lie 64 or more apart)"""
    px = np.array([[[255, 0, 128], [230, 20, 100], [96, 96, 96], [64, 128, 0], [224, 31, 159], [33, 222, 97]]] * 3, np.uint8)
    for k in range(5):
        f = bgra.with_alpha(px, k)
        assert bgra.apart(f) >= bgra.ALPHA_GAP
        for y in range(px.shape[0]):
            for x in range(px.shape[1]):
                order = [bgra.ALPHA_CANDIDATES[(x + y + k + i) % 4] for i in range(4)]
                want = next(a for a in order if all(abs(a - int(v)) >= 32 for v in px[y, x]))
                assert f[y, x, 3] == want, (k, y, x)
    assert (bgra.with_alpha(px, 0)[:, [0, 4], 3] == 64).all()          # three candidates blocked: the one that remains


@pytest.mark.parametrize("pad", bgra.PADS)
def test_padded_keeps_the_pixels(pad):
    f = bgra.with_alpha(hostile_frame("noise", 37, 53, 1), 1)
    v = bgra.padded(f, pad)
    step = 53 * 4 + pad
    assert v.strides == (step, 4, 1) and v.shape == f.shape and np.array_equal(v, f) and not v.flags["C_CONTIGUOUS"]
    flat = bgra.frame_bytes(v)
    assert flat.size == 36 * step + 53 * 4 and flat.ctypes.data == v.ctypes.data
    rows = np.concatenate([flat, np.full(pad, bgra.PAD_BYTE, np.uint8)]).reshape(37, step)
    assert np.array_equal(rows[:, :53 * 4].reshape(37, 53, 4), f) and (rows[:-1, 53 * 4:] == bgra.PAD_BYTE).all()
    if pad == 6:                                          # rows start at 2 mod 4: none but the first (and every other) is 4-byte aligned
        assert [(r * step) % 4 for r in range(4)] == [0, 2, 0, 2]


def hi_tap_from_alpha(alpha):
    """map_model.warp_linear_reflect_inv with one change: where the "lo" tap lies in the frame's last column but one, the "hi" tap
    (the last column) reads that pixel's alpha byte in all three channels -- what an 8-byte load of the row's last two BGRA pixels gives
    when its high half is unpacked a byte too far"""
    true_warp = map_model.warp_linear_reflect_inv

    def warp(src, M, drows, dcols, as_float, XY=None):
        base = true_warp(src, M, drows, dcols, as_float, XY)
        leak = src.copy()
        a = alpha.astype(np.float32) * np.float32(1. / 255.) if as_float else alpha.astype(src.dtype)
        leak[:, -1, :] = a[:, -1, None]
        X, _ = XY if XY is not None else map_model._warp_coords(M, drows, dcols, (32.0,))[0]
        sx = np.mod(np.clip(X >> 5, -32768, 32767), 2 * src.shape[1])
        return np.where((sx == src.shape[1] - 2)[..., None], true_warp(leak, M, drows, dcols, as_float, XY), base)
    return warp


def differs_at_level_0(a, b):
    assert a.tiles() == b.tiles()
    return sum(int((a.tile_level(*t, 0)[0] != b.tile_level(*t, 0)[0]).any(axis=2).sum()) for t in a.tiles())


@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_both_mutants_change_the_map(orc, kind, monkeypatch):
    """ModelMap (int16, 5 bands) on the four lattice keyframes of test_gpu_model.witnesses, fed [:3] of the BGRA frames (the truth: the
    model of witnesses itself), [1:4] (the slipped gather) and [:3] with the alpha-reading hi tap: both differ from the truth at level 0"""
    wl_poses, prep, frames, o, m = witnesses(kind, 0, 5)
    four = [bgra.with_alpha(f, k) for k, f in enumerate(frames)]
    slip, leak = ModelMap(band_num=5, force_float=0, bg_color=BG), ModelMap(band_num=5, force_float=0, bg_color=BG)
    o2 = orc.OracleMap(band_num=5, force_float=0, bg_color=BG)
    assert o2.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    true_warp = map_model.warp_linear_reflect_inv
    for f, p in zip(four, wl_poses):
        assert o2.feed(np.ascontiguousarray(f[:, :, :3]), p)
        dims, M = o2.last_canvas()
        slip.feed(np.ascontiguousarray(f[:, :, 1:4]), o2.grid(), o2.footprint(p), M)
        monkeypatch.setattr(map_model, "warp_linear_reflect_inv", hi_tap_from_alpha(f[:, :, 3]))
        leak.feed(np.ascontiguousarray(f[:, :, :3]), o2.grid(), o2.footprint(p), M)
        monkeypatch.setattr(map_model, "warp_linear_reflect_inv", true_warp)
        assert slip.last[0] == dims and leak.last[0] == dims
    assert o2.grid() == o.grid()
    n_slip, n_leak = differs_at_level_0(slip, m), differs_at_level_0(leak, m)
    print("%s: level-0 pixels changed by the slipped gather %d, by the alpha hi tap %d" % (kind, n_slip, n_leak))
    assert n_slip > 0 and n_leak > 0
