"""Views of injected pyramids (view_inject.py) without a device: the claim a view's plan rests on -- the window's pixels of the collapse
of the plan's rectangle of tiles ALONE equal the whole mosaic's -- on maps that no keyframe leaves behind (holes inside the rectangle,
maps one tile wide or high, rails and saturating collapses, tile coordinates outside the prepared grid); and the conditions the inputs
of tests/test_gpu_view_inject.py must meet to bite: weights that tell `w != 0` from the rules a kernel could apply instead, inside the
windows of the very views the GPU test renders, and lone pixels whose warped coverage falls on both sides of the paint rule."""
import numpy as np
import pytest

import pyramid_inject as pi
import view_inject as vi
from level_view_model import collapse_from
from map_model import to_8u
from view_model import ELE, extent_of, view_model

BG = pi.BG
# a grid that was prepared elsewhere: 4 x 3 tiles from stable tile (4, 5), so every tile of pi.SHAPES lies outside it and has a
# negative (tx - off_x), (ty - off_y) in A_k; lengthPixel 0.05 m, eleSize 256 lengthPixel, the minimum off any round number
SYNTHETIC_GRID = ([4, 3, 4, 5], [-7.3, 2.1, -7.3 + 4 * 12.8, 2.1 + 3 * 12.8, 12.8, 0.05])
# one rail kind and one colour kind per pyramid type; the kind of a case alternates with the band count and the shape
LAPS = {0: ("rails", "view"), 1: ("big", "view")}


def collapse_rectangle(m, rect, k):
    """save() at level k of the tiles inside rect alone: levels k .. L pasted (absent tiles zero), one collapse, the 8U view, bg_color
    where the level-k weight is 0"""
    tx, ty, nx, ny = rect
    lv = [None] * k + [np.zeros((ny * (ELE >> i), nx * (ELE >> i), 3), m.dtype) for i in range(k, m.L + 1)]
    wk = np.zeros((ny * (ELE >> k), nx * (ELE >> k)), np.float32)
    for (ix, iy), (lap, wts) in m.tiles_.items():
        if not (tx <= ix < tx + nx and ty <= iy < ty + ny):
            continue
        for i in range(k, m.L + 1):
            s = ELE >> i
            lv[i][(iy - ty) * s:(iy - ty + 1) * s, (ix - tx) * s:(ix - tx + 1) * s] = lap[i]
        e = ELE >> k
        wk[(iy - ty) * e:(iy - ty + 1) * e, (ix - tx) * e:(ix - tx + 1) * e] = wts[k]
    out = to_8u(collapse_from(lv, k))
    out[wk == 0] = np.uint8(BG)
    return out


def window_pixels(img, info):
    x0, y0, w, h = info["window"]
    return img[y0:y0 + h, x0:x0 + w]


# ---------------------------------------------------------------- 1. the plan's claim
@pytest.mark.parametrize("shape", ["nine", "holes", "row", "column"])
@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
def test_the_rectangles_collapse_equals_the_whole_mosaics_on_the_window(pf, force_float, bands, shape):
    """per level of {0, 1, bands // 2, bands}: a tile's first column, its last column, and four seeded crops"""
    n_shape = ["nine", "holes", "row", "column"].index(shape)
    lap_kind = LAPS[force_float][(n_shape + bands) % 2]
    tiles, _ = pi.make_tiles(bands, force_float, shape, lap_kind, "half", 11)
    m = pi.model_of(tiles, bands, force_float)
    dims, geo = SYNTHETIC_GRID
    ex = extent_of(m.tiles())
    assert ex[0] - dims[2] < 0 and ex[1] - dims[3] < 0                 # A_k's (tx - off_x), (ty - off_y) are negative
    rng = np.random.RandomState(100 * bands + 10 * n_shape + force_float)
    smaller = cases = 0
    for k in sorted({0, 1, bands // 2, bands}):
        e = ELE >> k
        S, C, origin = vi.truth_of(m, k)
        for n in range(6):
            w, h = (1, e) if n < 2 else (int(rng.randint(1, 2 * e + 2)), int(rng.randint(1, e + 2)))
            ax = int(rng.randint(-3, ex[2] * e)) if n > 1 else (0 if n == 0 else e - 1)          # the first tile's first column, its last one, then anywhere
            ay = int(rng.randint(-3, ex[3] * e)) if n > 1 else 0
            info = pf.view_plan(vi.crop_view(SYNTHETIC_GRID, ex, k, ax, ay), w, h, k, dims, geo, m.num_levels, ex)
            if info["empty"]:
                continue
            cases += 1
            tx, ty, nx, ny = info["rect"]
            assert ex[0] <= tx and ex[1] <= ty and tx + nx <= ex[0] + ex[2] and ty + ny <= ex[1] + ex[3]
            smaller += nx * ny < ex[2] * ex[3]
            sub = collapse_rectangle(m, info["rect"], k)
            x0, y0 = (tx - origin[0]) * e, (ty - origin[1]) * e
            whole = S[y0:y0 + ny * e, x0:x0 + nx * e]
            assert np.array_equal(window_pixels(sub, info), window_pixels(whole, info)), (k, n, info["rect"], info["window"])
    assert cases >= 8
    if shape != "nine" or bands < 8:
        # (nine tiles at eight bands: two tiles of ring around any window are the whole 3 x 3)
        assert smaller > 0, "no rectangle was smaller than the extent"


def test_the_views_model_reads_the_window_alone(pf):
    """the model warps the crop of the whole mosaic; with every pixel of the rectangle outside the window replaced by noise, coverage
    255, the view is the same -- on a map with holes, through a seeded homography and a crop"""
    m = vi.model(5, 0, "holes", "view", "nonfinite", 3)
    ex = extent_of(m.tiles())
    rng = np.random.RandomState(5)
    views = [(V, 150, 37) for V in vi.seeded_views(SYNTHETIC_GRID, ex, 31, 3)] + [(vi.crop_view(SYNTHETIC_GRID, ex, 1, 100, 90), 64, 48)]
    for k in (0, 1, 3):
        e = ELE >> k
        S, C, origin = vi.truth_of(m, k)
        for V, w, h in views:
            info = pf.view_plan(V, w, h, k, SYNTHETIC_GRID[0], SYNTHETIC_GRID[1], m.num_levels, ex)
            assert not info["empty"]
            tx, ty, nx, ny = info["rect"]
            x0, y0 = (tx - origin[0]) * e, (ty - origin[1]) * e
            wx0, wy0, ww, wh = info["window"]
            keep = np.zeros((ny * e, nx * e), bool); keep[wy0:wy0 + wh, wx0:wx0 + ww] = True
            S2, C2 = S.copy(), C.copy()
            S2[y0:y0 + ny * e, x0:x0 + nx * e][~keep] = rng.randint(0, 256, (int((~keep).sum()), 3))
            C2[y0:y0 + ny * e, x0:x0 + nx * e][~keep] = 255
            assert np.array_equal(view_model(S, C, origin, info, w, h, BG), view_model(S2, C2, origin, info, w, h, BG)), (k, info["window"])


def test_truth_is_kept_on_the_model_not_by_id():
    a = vi.model(1, 0, "one", "view", "half", 1)
    Sa = vi.truth_of(a, 0)[0]
    assert vi.truth_of(a, 0)[0] is Sa and a._view_truth[0][0] is Sa
    b = vi.model(1, 0, "one", "view", "half", 2)
    assert "_view_truth" not in b.__dict__ and not np.array_equal(vi.truth_of(b, 0)[0], Sa)


# ---------------------------------------------------------------- 2. the inputs can tell the rules apart
def test_nonfinite_weights_are_what_they_say():
    tiles, kinds = vi.make_tiles(5, 1, "holes", "view", "nonfinite", 12)
    half, _ = pi.make_tiles(5, 1, "holes", "view", "half", 12)
    assert set(kinds.values()) == {"nonfinite"}
    for t, (_, w) in tiles.items():
        for i, a in enumerate(w):
            h = half[t][1][i]
            bits = a.view(np.uint32)
            assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any() and (bits == 0x80000000).any(), (t, i)
            assert np.array_equal(a != 0, h != 0)                                              # the coverage is the `half` tile's
            odd = ~np.isfinite(a)
            assert int(odd.sum()) == max(3, int((h != 0).sum()) // 8) and np.array_equal(a[~odd & (a != 0)], h[~odd & (a != 0)])
            assert int((bits == 0x80000000).sum()) == max(1, int((h == 0).sum()) // 8)


def level0_read_at_level_k(m, k):
    """what `w_off[0]` for `w_off[k]` reads: the tile's level-0 plane under the level-k index, the first (256 >> k)^2 floats"""
    x0, y0, nx, ny = extent_of(m.tiles())
    e = ELE >> k
    out = np.zeros((ny * e, nx * e), np.float32)
    for (ix, iy), (_, w) in m.tiles_.items():
        out[(iy - y0) * e:(iy - y0 + 1) * e, (ix - x0) * e:(ix - x0 + 1) * e] = w[0].reshape(-1)[:e * e].reshape(e, e)
    return out


@pytest.mark.parametrize("w_kind", ["signs", "nonfinite"])
@pytest.mark.parametrize("force_float", [0, 1])
def test_the_weights_tell_the_rule_from_the_wrong_ones(pf, force_float, w_kind):
    """For the maps of the GPU test's weight cases (which its ways out use too), at every level, inside the windows of the views it
    renders at that level: each wrong rule a kind can show (view_inject.TELLS: `signs` holds no NaN, `nonfinite` no denormal; between
    them all of `w > 0`, `|w| >= FLT_MIN`, `w == w and w != 0`) disagrees with `w != 0` on a pixel, and so do the level-0 weights
    decimated to level k and the level-0 plane read under the level-k index.  No level is left out: at 5 bands the top level still
    has 8 x 8 pixels a tile."""
    args = vi.weight_map_args(force_float, w_kind)
    m = vi.model(*args)
    grid = vi.grid_of(args[0])
    dims, geo = grid
    ex = extent_of(m.tiles())
    inside = {k: np.zeros(vi.weights_of(m, k).shape, bool) for k in range(m.num_levels)}
    for level, V, w, h, _ in vi.weight_views(grid, m):
        info = pf.view_plan(V, w, h, level, dims, geo, m.num_levels, ex)
        if info["empty"]:
            continue
        e = ELE >> info["level"]
        x0, y0 = (info["rect"][0] - ex[0]) * e + info["window"][0], (info["rect"][1] - ex[1]) * e + info["window"][1]
        inside[info["level"]][y0:y0 + info["window"][3], x0:x0 + info["window"][2]] = True
    w0 = vi.weights_of(m, 0)
    for k in range(m.num_levels):
        wk = vi.weights_of(m, k)
        right = wk != 0
        assert inside[k].any(), k
        for name in vi.TELLS[w_kind]:
            with np.errstate(invalid="ignore"):
                wrong = vi.WRONG_RULES[name](wk)
            assert ((wrong != right) & inside[k]).any(), (k, name)
        if k:
            assert (((w0[::1 << k, ::1 << k] != 0) != right) & inside[k]).any(), (k, "decimated")
            assert (((level0_read_at_level_k(m, k) != 0) != right) & inside[k]).any(), (k, "level 0 under the level-k index")
    assert set(vi.TELLS["signs"]) | set(vi.TELLS["nonfinite"]) == set(vi.WRONG_RULES)


# ---------------------------------------------------------------- 3. the lone pixels
@pytest.mark.parametrize("w_kind", ["lone_one", "lone_zero"])
def test_lone_pixels_fall_on_both_sides_of_the_paint_rule(pf, w_kind):
    """Scale 1 shifted by (a / 32, b / 32).  A lone covered pixel is the last tap of view pixel (2, 2) with the weight a b 32 of 32768:
    (255 a b 32 + 16384) >> 15 is 0 for a b <= 2 -- at (1, 1), (1, 2), (2, 1) a covered tap of positive weight rounds away and the
    pixel is painted -- and not 0 from a b = 3 on.  A lone uncovered pixel is the first tap of view pixel (3, 3): coverage 0 only at
    the shift (0, 0), where the other taps weigh 1 together; at any other shift the colour interpolated from it is kept."""
    m = vi.model(5, 0, "holes", "view", w_kind, vi.LONE_SEED)
    grid = vi.grid_of(5)
    assert vi.lone_pixel(m) == (31, 7)
    w, h = vi.LONE_SIZE
    painted = kept = rounded_away = 0
    u = 2 if w_kind == "lone_one" else 3
    for a, b in vi.LONE_SHIFTS:
        got, plan = vi.model_view(pf, grid, m, vi.lone_view(grid, m, a, b), w, h, 0)
        assert abs(plan["M0"][0, 0] - 1) < 1e-12 and abs(plan["M0"][0, 2] * 32 - round(plan["M0"][0, 2] * 32)) < 1e-6          # on the 1 / 32 grid, off every tie
        zero = got[u, u, 3] == 0
        if w_kind == "lone_one":
            assert zero == (a * b <= 2), (a, b)
            assert int((got[:, :, 3] != 0).sum()) <= 4
            rounded_away += bool(zero and a * b > 0)
        else:
            assert zero == ((a, b) == (0, 0)), (a, b)
        if zero:
            assert (got[u, u, :3] == BG).all()
        painted += int(zero); kept += int(not zero)
    assert painted > 0 and kept > 0
    if w_kind == "lone_one":
        assert rounded_away >= 3
