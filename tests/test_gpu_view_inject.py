"""Rendered views (csrc/view.hip, map_view.cpp, view_plan.hpp behind pf_render_view*) of stored state that no keyframe leaves behind
(pyramid_inject.py, view_inject.py), against the model on the very arrays that were imported, byte for byte over every pixel.  Pinned
here: k_view_cover's zero test at every level (-0.0, denormals, negative weights, NaN, the infinities, whole tiles of zeros, lone
pixels) through a tile table with zero entries; absent tiles inside the collapsed rectangle and rectangles narrower than the extent;
the paint rule on lone pixels under sub-pixel shifts; general views at 0, 1, 2 and 8 bands on maps one tile wide or high; saturating
collapses under a view; extents with negative tile coordinates; source coordinates beyond the short and the int range.
tests/test_view_inject_model.py checks on the host that these inputs can tell the rules apart."""
import numpy as np
import pytest

import pyramid_inject as pi
import view_inject as vi
from view_inject import check_view, check_view_padded, render_checked
from view_model import ELE, extent_of

pytestmark = pytest.mark.gpu

BG = pi.BG
FULL = {0: "full", 1: "wide"}


def outside_the_grid(g, m):
    """the imported tiles lie outside the prepared grid: A_k has a negative (tx - off_x) or (ty - off_y)"""
    dims, _ = g.grid()
    ex = extent_of(m.tiles())
    return ex[0] - dims[2] < 0 or ex[1] - dims[3] < 0


# ---------------------------------------------------------------- 1. weights, every level
WEIGHT_MODELS = {}          # by (type, weight kind): the two cases of a map share the model and its truth, which they leave unchanged


@pytest.mark.parametrize("asked", ["level", "auto"])
@pytest.mark.parametrize("w_kind", vi.WEIGHT_KINDS)
@pytest.mark.parametrize("ff", [0, 1])
def test_every_weight_kind_at_every_level_of_a_map_with_holes(pf, ff, w_kind, asked):
    """crops at scale 1 at level k, asked at level k (`level`) or at -1 (`auto`): each is the crop of S_k and C_k outright, and the
    model's; they start and end on tile borders, lie over the hole and the absent column, leave the extent.  Two general homographies
    at every explicit level, or at -1."""
    args = vi.weight_map_args(ff, w_kind)
    if (ff, w_kind) not in WEIGHT_MODELS:
        WEIGHT_MODELS[(ff, w_kind)] = vi.model(*args)
    m = WEIGHT_MODELS[(ff, w_kind)]
    g = vi.map_of(pf, m, args[0], ff)
    grid = g.grid()
    assert [list(grid[0]), list(grid[1])] == [list(a) for a in vi.grid_of(args[0])]          # the host-side conditions were checked on these very views
    assert outside_the_grid(g, m)
    sub = outright = 0
    chosen = set()
    for level, V, w, h, crop in vi.weight_views(grid, m):
        if (level < 0) != (asked == "auto"):
            continue
        got, info = render_checked(pf, g, m, V, w, h, level)
        sub += (not info["empty"]) and info["tiles"] < 15
        if level < 0:
            chosen.add(info["level"])
        if crop is not None:
            assert info["level"] == crop[0], (level, crop, "scale 1 at level k is a dyadic scale: level -1 takes level k")
            S, Cv, _ = vi.truth_of(m, info["level"])
            want, inside = vi.crop_of_truth(S, Cv, crop[1], crop[2], w, h)
            assert np.array_equal(got, want), (info["level"], crop)
            assert info["empty"] == (not inside)
            if info["empty"]:
                assert info["tiles"] == 0
            outright += 1
    assert sub > 0                                                       # rectangles narrower than the extent, with table entries of 0
    assert outright == 6 * m.num_levels
    assert chosen == (set(range(m.num_levels)) if asked == "auto" else set())
    g.close()


# ---------------------------------------------------------------- 2. lone pixels under sub-pixel shifts
@pytest.mark.parametrize("w_kind", ["lone_one", "lone_zero"])
def test_lone_pixels_under_sub_pixel_shifts(pf, w_kind):
    """the views of tests/test_view_inject_model.py: their warped coverage is 0 at some shifts (painted) and not at others (the
    interpolated colour kept); four channels, and three into rows with padding"""
    g, m = vi.build(pf, 5, 0, "holes", "view", w_kind, vi.LONE_SEED)
    grid = g.grid()
    w, h = vi.LONE_SIZE
    u = 2 if w_kind == "lone_one" else 3
    painted = kept = 0
    for a, b in vi.LONE_SHIFTS:
        V = vi.lone_view(grid, m, a, b)
        got, _ = render_checked(pf, g, m, V, w, h, 0)
        check_view_padded(pf, g, m, V, w, h, 0)
        painted += int(got[u, u, 3] == 0); kept += int(got[u, u, 3] != 0)
        if got[u, u, 3] == 0:
            assert (got[u, u, :3] == BG).all()
    assert painted > 0 and kept > 0
    g.close()


# ---------------------------------------------------------------- 3. bands and shapes
BAND_CASES = [(bands, ff, shape, "view") for bands in (0, 1, 2, 8) for ff in (0, 1) for shape in ("one", "row", "column", "nine")]
BAND_CASES += [(8, ff, shape, FULL[ff]) for ff in (0, 1) for shape in ("one", "row", "column", "nine")]


@pytest.mark.parametrize("bands,ff,shape,lap_kind", BAND_CASES)
def test_general_views_at_every_band_count_and_shape(pf, bands, ff, shape, lap_kind):
    """four seeded homographies at every explicit level and at -1, 150 x 37 and 40 x 5"""
    g, m = vi.build(pf, bands, ff, shape, lap_kind, "half", 3)
    grid = g.grid()
    assert m.num_levels == bands + 1 and outside_the_grid(g, m)
    ex = extent_of(m.tiles())
    seen = 0
    for V in vi.seeded_views(grid, ex, 41 + bands, 4):
        for level in [-1] + list(range(m.num_levels)):
            for w, h in ((150, 37), (40, 5)):
                info = check_view(pf, g, m, V, w, h, level)
                seen += not info["empty"]
        check_view_padded(pf, g, m, V, 150, 37, -1)
    assert seen > 0
    g.close()


@pytest.mark.parametrize("shape", ["row", "column"])
@pytest.mark.parametrize("ff", [0, 1])
def test_one_pixel_views_at_eight_bands_on_maps_one_tile_wide_or_high(pf, ff, shape):
    """One pixel wide and one tile high on the first tile's first and last column, one pixel high and one tile wide on its first and
    last row, at levels 0, 3, 5 and 7: along the map the ring is two tiles (a rectangle of three of the row's five, of the column's
    four), across it the rectangle is the extent's one tile.  The level mosaics of such rectangles have rows or columns that are no
    multiple of the collapse's blocks (128 x 32): the clipped blocks run on a sub-rectangle."""
    g, m = vi.build(pf, 8, ff, shape, "view", "half", 5)
    grid = g.grid()
    ex = extent_of(m.tiles())
    along, across = (0, 1) if shape == "row" else (1, 0)
    clipped = 0
    for k in (0, 3, 5, 7):
        e = ELE >> k
        for n, (ax, ay, w, h) in enumerate(((0, 0, 1, e), (e - 1, 0, 1, e), (0, 0, e, 1), (0, e - 1, e, 1))):
            info = check_view(pf, g, m, vi.crop_view(grid, ex, k, ax, ay), w, h, k)
            rect = info["rect"]
            assert rect[0] == ex[0] and rect[1] == ex[1] and rect[2 + across] == ex[2 + across] == 1
            assert rect[2 + along] < ex[2 + along], (k, n, rect, ex)
            if k == 0 and n == (1 if shape == "row" else 3):
                assert rect[2 + along] == 3, (rect, "the last column or row: two tiles of ring behind it")
            if k and ((rect[2] * e) % 128 or (rect[3] * e) % 32):
                clipped += 1
    assert clipped > 0
    g.close()


# ---------------------------------------------------------------- 4. saturating collapses under a view
@pytest.mark.parametrize("ff,lap_kind", [(0, "rails"), (0, "opposed"), (1, "big"), (1, "ties")])
def test_saturating_collapses_under_a_view(pf, ff, lap_kind):
    """the collapse that feeds a view is save's: 16S sums that leave the range, 32F values far outside [0, 1] and on the ties of the 8U
    view.  Two homographies at levels 0, 2 and L"""
    g, m = vi.build(pf, 5, ff, "nine", lap_kind, "half", 1)
    grid = g.grid()
    ex = extent_of(m.tiles())
    for V in vi.seeded_views(grid, ex, 61, 2):
        for level in (0, 2, m.num_levels - 1):
            info = check_view(pf, g, m, V, 150, 37, level)
            assert not info["empty"]
    g.close()


# ---------------------------------------------------------------- 5. far coordinates
@pytest.mark.parametrize("ff", [0, 1])
def test_source_coordinates_beyond_the_short_and_the_int_range(pf, ff):
    """view_inject.far_views, 64 x 48, level 0 forced and level -1 (which is the top level at these pitches): the convert to int that
    saturates, then sat_short, against the oracle's warp, which restates both clamps.  The plan takes every one of them (the window is
    clipped to the extent before a region is sized): pitches of 3000 and of 2e6 level-0 pixels as asked."""
    g, m = vi.build(pf, 5, ff, "nine", "view", "half", 8)
    grid = g.grid()
    ex = extent_of(m.tiles())
    for name, V in vi.far_views(grid, ex).items():
        for level in (0, -1):
            got, info = render_checked(pf, g, m, V, 64, 48, level)
            assert not info["empty"] and tuple(info["rect"]) == tuple(ex), (name, info["rect"])
            if name != "fivefold":
                assert info["level"] == (0 if level == 0 else m.num_levels - 1)
            covered = got[:, :, 3] != 0
            assert covered.any() and not covered.all(), name
            assert not covered[0].any() and not covered[:, 0].any(), (name, "the content lies under interior pixels")
            # X of the last view pixel, in 1 / 32 of a level pixel: where it lies against the two ranges
            M = np.asarray(info["Minv"]).reshape(3, 3)
            X = 32.0 * (M[0, 0] * 63 + M[0, 1] * 47 + M[0, 2]) / (M[2, 0] * 63 + M[2, 1] * 47 + M[2, 2])
            if name == "short" and level == 0:
                assert 32 * 32767 < X < 2.0 ** 31
            if name == "int":
                assert X > (2.0 ** 31 if level == 0 else 32 * 32767)
        check_view_padded(pf, g, m, V, 64, 48, 0)
    g.close()


# ---------------------------------------------------------------- 6. one of each way out
def test_ways_out_of_a_map_with_hostile_weights(pf):
    import torch
    g, m = vi.build(pf, *vi.weight_map_args(0, "signs"))
    grid = g.grid()
    V = vi.seeded_views(grid, extent_of(m.tiles()), vi.WEIGHT_VIEW_SEED, 2)[1]
    w, h = 150, 37
    host4, info = render_checked(pf, g, m, V, w, h, -1)
    host3, _ = render_checked(pf, g, m, V, w, h, -1, 3)
    assert not info["empty"] and (host4[:, :, 3] == 0).any() and (host4[:, :, 3] != 0).any()
    for channels, host in ((4, host4), (3, host3)):
        step = w * channels + 12
        padded = torch.full((h, step), vi.SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                         # the map works on a stream of its own: the fill comes first
        assert g.render_view_device(V, w, h, padded.data_ptr(), -1, channels, step=step)["rect"] == info["rect"]
        back = padded.cpu().numpy()
        assert np.array_equal(back[:, :w * channels].reshape(h, w, channels), host) and (back[:, w * channels:] == vi.SENTINEL).all()
    stream, jinfo = g.render_view_jpeg(V, w, h, -1, 95)
    assert stream == pf.jpeg_encode(host3, 95) and jinfo["rect"] == info["rect"]
    g.close()
