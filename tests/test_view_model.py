"""The claim a view's plan rests on, checked on the host with the oracle's maps: the pixels of the plan's window, taken from the collapse
of the plan's rectangle of tiles ALONE (its edges treated as image edges, as the kernels treat them), equal those of the whole
mosaic's collapse -- so the view warped from the rectangle is the view warped from the whole save().  And the ring is not too large:
with the rectangle shrunk by one tile where eight bands need two, the window's pixels change.  No device."""
import numpy as np
import pytest

from level_view_model import collapse_from
from map_model import to_8u
from view_model import BG, ELE, extent_of, held_tiles, oracle_map, truth, view_model


def collapse_rectangle(o, rect, k):
    """save() at level k of the tiles inside rect alone: levels k .. L pasted (absent tiles zero), one collapse, the 8U view, bg_color
    where the level-k weight is 0"""
    held = held_tiles(o)
    L = o.num_levels - 1
    tx, ty, nx, ny = rect
    lv = [None] * k + [np.zeros((ny * (ELE >> i), nx * (ELE >> i), 3), o.dtype) for i in range(k, L + 1)]
    wk = np.zeros((ny * (ELE >> k), nx * (ELE >> k)), np.float32)
    for (ix, iy), (lap, wts) in held.items():
        if not (tx <= ix < tx + nx and ty <= iy < ty + ny):
            continue
        for i in range(k, L + 1):
            s = ELE >> i
            lv[i][(iy - ty) * s:(iy - ty + 1) * s, (ix - tx) * s:(ix - tx + 1) * s] = lap[i]
        e = ELE >> k
        wk[(iy - ty) * e:(iy - ty + 1) * e, (ix - tx) * e:(ix - tx + 1) * e] = wts[k]
    out = to_8u(collapse_from(lv, k))
    out[wk == 0] = np.uint8(BG)
    return out


def crop_view(o, k, ax, ay):
    """V of scale 1 at level k: view pixel (u, v) over level-k pixel (u + ax, v + ay) of the extent"""
    dims, geo = o.grid()
    ex = extent_of(o.tiles())
    s = geo[5] * (1 << k)
    ox, oy = geo[0] + (ex[0] - dims[2]) * geo[4], geo[1] + (ex[1] - dims[3]) * geo[4]
    return np.array([[1 / s, 0, -ox / s - ax], [0, 1 / s, -oy / s - ay], [0, 0, 1.0]])


def plan_of(pf, o, V, w, h, level):
    dims, geo = o.grid()
    return pf.view_plan(V, w, h, level, dims, geo, o.num_levels, extent_of(o.tiles()))


def window_pixels(img, info):
    x0, y0, w, h = info["window"]
    return img[y0:y0 + h, x0:x0 + w]


@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("bands", [1, 5, 8])
def test_the_rectangles_collapse_equals_the_whole_mosaics_on_the_window(pf, force_float, bands):
    o = oracle_map(force_float, bands)
    ex = extent_of(o.tiles())
    rng = np.random.RandomState(bands)
    smaller = 0
    for k in sorted({0, 1, bands // 2, bands}):
        e = ELE >> k
        S, C, origin = truth(o, k)
        for n in range(6):
            w, h = (1, e) if n == 0 else (e, 1) if n == 1 else (int(rng.randint(1, 2 * e + 2)), int(rng.randint(1, e + 2)))
            ax = int(rng.randint(-3, ex[2] * e)) if n > 2 else (1 + n) * e - (n % 2)          # a tile's first column, the last one, then anywhere
            ay = int(rng.randint(-3, ex[3] * e)) if n > 2 else e
            info = plan_of(pf, o, crop_view(o, k, ax, ay), w, h, k)
            if info["empty"]:
                continue
            tx, ty, nx, ny = info["rect"]
            smaller += nx * ny < ex[2] * ex[3]
            sub = collapse_rectangle(o, info["rect"], k)
            x0, y0 = (tx - origin[0]) * e, (ty - origin[1]) * e
            whole = S[y0:y0 + ny * e, x0:x0 + nx * e]
            assert np.array_equal(window_pixels(sub, info), window_pixels(whole, info)), (k, n, info["rect"], info["window"])
            # ... and the view's model, which warps the crop of the whole mosaic, reads nothing else: the crop's other pixels may be anything
            noise = whole.copy(); cov = C[y0:y0 + ny * e, x0:x0 + nx * e].copy()
            wx0, wy0, ww, wh = info["window"]
            keep = np.zeros(noise.shape[:2], bool); keep[wy0:wy0 + wh, wx0:wx0 + ww] = True
            noise[~keep] = rng.randint(0, 256, (int((~keep).sum()), 3)); cov[~keep] = 255
            S2, C2 = S.copy(), C.copy()
            S2[y0:y0 + ny * e, x0:x0 + nx * e] = noise; C2[y0:y0 + ny * e, x0:x0 + nx * e] = cov
            a, b = view_model(S, C, origin, info, w, h, BG), view_model(S2, C2, origin, info, w, h, BG)
            assert np.array_equal(a, b), (k, n, info["window"])
    assert smaller > 0


def test_one_tile_of_ring_is_not_enough_at_eight_bands(pf):
    """a view one pixel wide and one tile high on a tile's last column: at eight bands the plan takes two tiles to its right, and with one
    of them taken away the window's pixels are no longer the whole mosaic's -- the ring is as small as it may be"""
    o = oracle_map(0, 8)
    tiles = set(o.tiles())
    ex = extent_of(o.tiles())
    S, C, origin = truth(o, 0)
    t = sorted(t for t in tiles if (t[0] + 1, t[1]) in tiles and (t[0] + 2, t[1]) in tiles)[0]
    ax, ay = (t[0] - ex[0] + 1) * ELE - 1, (t[1] - ex[1]) * ELE
    info = plan_of(pf, o, crop_view(o, 0, ax, ay), 1, ELE, 0)
    tx, ty, nx, ny = info["rect"]
    assert tx + nx - 1 == t[0] + 2, info["rect"]
    whole = S[(ty - origin[1]) * ELE:(ty - origin[1] + ny) * ELE, (tx - origin[0]) * ELE:(tx - origin[0] + nx) * ELE]
    assert np.array_equal(window_pixels(collapse_rectangle(o, info["rect"], 0), info), window_pixels(whole, info))
    short = collapse_rectangle(o, (tx, ty, nx - 1, ny), 0)
    x0, y0, w, h = info["window"]
    assert not np.array_equal(short[y0:y0 + h, x0:x0 + w], whole[y0:y0 + h, x0:x0 + w]), "a ring of one tile gave the same pixels"
