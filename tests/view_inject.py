"""Rendered views (pf_render_view*, DESIGN.md "Views") of pyramids put straight into the tile slots (pyramid_inject.py), test code only:
the truth of an injected ModelMap at every level, a weight kind of its own with NaN, the infinities and -0.0, the check of one view
against the model, and the makers of the views.  A view of an injected map is the oracle's warp of the crop of the model's
whole-mosaic collapse (view_model.py); tests/test_view_inject_model.py checks on the host that the plan's claim holds for such maps.

Nothing here needs a GPU to import; build() does."""
import numpy as np

import pyramid_inject as pi
from view_model import ELE, coverage_of, extent_of, view_model

SENTINEL = 0xA5
FLT_MIN = np.float32(1.17549435e-38)
# the zero tests k_view_cover could apply instead of the IEEE `w != 0` (C_k is 255 where weights[k] != 0)
WRONG_RULES = {
    "positive": lambda w: w > 0,                                    # drops negative weights, -inf and NaN
    "flushed": lambda w: np.abs(w) >= FLT_MIN,                      # denormals flushed to zero (NaN compares false: dropped as well)
    "ordered": lambda w: (w == w) & (w != 0),                       # an ordered comparison: NaN dropped
}
# which of them a weight kind can tell from the rule: `signs` holds no NaN, `nonfinite` no denormal
TELLS = {"signs": ("positive", "flushed"), "nonfinite": ("positive", "ordered")}


# ---------------------------------------------------------------- the weight kind `nonfinite`
def nonfinite_weights(w, rng):
    """[w_0 .. w_L] of a `half` tile with, at every level, a seeded eighth of the entries that are not zero replaced by NaN, +inf and
    -inf in turn (at least one of each where the level has three such entries) and a seeded eighth of the zeros by -0.0 (at least one).
    By `w != 0` NaN and the infinities are covered and -0.0 is not."""
    out = []
    for a in w:
        a = a.copy()
        flat = a.reshape(-1)
        nz, z = np.flatnonzero(flat != 0), np.flatnonzero(flat == 0)
        pick = rng.permutation(nz)[:min(nz.size, max(3, nz.size // 8))]
        flat[pick] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(pick.size) % 3]
        flat[rng.permutation(z)[:min(z.size, max(1, z.size // 8))]] = np.float32(-0.0)
        out.append(a)
    return out


def make_tiles(bands, force_float, shape, lap_kind, w_kind, seed):
    """pi.make_tiles, and the weight kind `nonfinite`: the `half` weights of every tile through nonfinite_weights, a stream per tile"""
    if w_kind != "nonfinite":
        return pi.make_tiles(bands, force_float, shape, lap_kind, w_kind, seed)
    tiles, kinds = pi.make_tiles(bands, force_float, shape, lap_kind, "half", seed)
    for j, t in enumerate(list(tiles)):
        tiles[t] = (tiles[t][0], nonfinite_weights(tiles[t][1], np.random.default_rng([seed, j, bands, 77])))
        kinds[t] = "nonfinite"
    return tiles, kinds


def model(bands, force_float, shape, lap_kind, w_kind, seed):
    """the ModelMap of make_tiles, with .w_kinds: no device"""
    tiles, kinds = make_tiles(bands, force_float, shape, lap_kind, w_kind, seed)
    m = pi.model_of(tiles, bands, force_float)
    m.w_kinds = kinds
    return m


def build(pf, bands, force_float, shape, lap_kind, w_kind, seed):
    """pi.build with the weight kinds of make_tiles: (map, model), the same arrays in both"""
    m = model(bands, force_float, shape, lap_kind, w_kind, seed)
    return map_of(pf, m, bands, force_float), m


def map_of(pf, m, bands, force_float):
    """pi.new_map with the model's own arrays imported"""
    g = pi.new_map(pf, bands, force_float)
    m.packed = pi.import_tiles(g, m.tiles_)
    assert g.tiles() == m.tiles()
    return g


# ---------------------------------------------------------------- the truth
def weights_of(m, k):
    """the level-k weights pasted over the extent, absent tiles zero"""
    x0, y0, nx, ny = extent_of(m.tiles())
    e = ELE >> k
    wk = np.zeros((ny * e, nx * e), np.float32)
    for (ix, iy), (_, w) in m.tiles_.items():
        wk[(iy - y0) * e:(iy - y0 + 1) * e, (ix - x0) * e:(ix - x0 + 1) * e] = w[k]
    return wk


def truth_of(m, k):
    """(S_k, C_k, origin) of a ModelMap: S_0 is its save(), S_k level_view_model's model_save_level; C_k the coverage of the level-k
    weights pasted over the extent.  Kept on the model itself and left unchanged: a cache keyed by id() would hand a new model the
    truth of a freed one."""
    from level_view_model import model_save_level
    cache = m.__dict__.setdefault("_view_truth", {})
    if k not in cache:
        S, origin = m.save() if k == 0 else model_save_level(m, k)
        wk = weights_of(m, k)
        assert origin == extent_of(m.tiles())[:2] and S.shape[:2] == wk.shape
        cache[k] = (S, coverage_of(wk), origin)
    return cache[k]


# ---------------------------------------------------------------- a view against the model
def grid_of(bands):
    """(dims, geo) of pi.new_map's grid without a device: the oracle prepared from the same plane, camera and poses"""
    if bands not in _GRIDS:
        from helpers import workloads
        from oracle import orc
        from test_gpu_model import CAM, lattice_poses
        o = orc.OracleMap(band_num=bands, force_float=0, bg_color=pi.BG)
        assert o.prepare(workloads().IDENTITY_PLANE, CAM, lattice_poses(11 + bands)[:2])
        dims, geo = o.grid()
        _GRIDS[bands] = (list(dims), list(geo))
    return _GRIDS[bands]


_GRIDS = {}


def model_view(pf, grid, m, V, width, height, level, channels=4):
    """(pixels, plan) of the model: the plan of the grid and of the model's extent, the oracle's warp of the crop of S_k and C_k"""
    dims, geo = grid
    plan = pf.view_plan(V, width, height, level, dims, geo, m.num_levels, extent_of(m.tiles()))
    S, Cv, origin = truth_of(m, plan["level"])
    return view_model(S, Cv, origin, plan, width, height, pi.BG, channels), plan


def render_checked(pf, g, m, V, width, height, level, channels=4, out=None):
    """one view against the model: (pixels, info)"""
    got, info = g.render_view(V, width, height, level, channels, out)
    want, plan = model_view(pf, g.grid(), m, V, width, height, level, channels)
    for key in ("level", "rect", "window", "empty", "tiles"):
        assert info[key] == plan[key], (key, info[key], plan[key])
    assert info["M0"].tobytes() == plan["M0"].tobytes() and info["Minv"].tobytes() == plan["Minv"].tobytes()
    assert got.shape == want.shape
    assert np.array_equal(got, want), (width, height, level, channels, info["rect"], int((got != want).any(axis=2).sum()), "pixels differ")
    return got, info


def check_view(pf, g, m, V, width, height, level, channels=4, out=None):
    """The returned info is the pure plan of the map's own grid, of the model's levels and of its tiles' extent; the pixels are the
    model's, every one.  Returns the info."""
    return render_checked(pf, g, m, V, width, height, level, channels, out)[1]


def check_view_padded(pf, g, m, V, width, height, level):
    """three channels into rows with five bytes of padding, which stay the caller's"""
    pad = np.full((height, width * 3 + 5), SENTINEL, np.uint8)
    info = check_view(pf, g, m, V, width, height, level, 3, pad[:, :width * 3].reshape(height, width, 3))
    assert (pad[:, width * 3:] == SENTINEL).all()
    return info


# ---------------------------------------------------------------- the makers of views
def extent_origin(grid, extent):
    """plane metres of the extent's first pixel"""
    dims, geo = grid
    return geo[0] + (extent[0] - dims[2]) * geo[4], geo[1] + (extent[1] - dims[3]) * geo[4]


def crop_view(grid, extent, k, ax, ay):
    """V of scale 1 at level k: view pixel (u, v) over level-k pixel (u + ax, v + ay) of the extent"""
    ox, oy = extent_origin(grid, extent)
    s = grid[1][5] * (1 << k)
    return np.array([[1 / s, 0, -ox / s - ax], [0, 1 / s, -oy / s - ay], [0, 0, 1.0]])


def pixel_view(grid, extent, M):
    """V of a matrix M from view pixels to level-0 pixels of the extent: V = inv(A_0 M)"""
    ox, oy = extent_origin(grid, extent)
    lp = grid[1][5]
    return np.linalg.inv(np.array([[lp, 0, ox], [0, lp, oy], [0, 0, 1.0]]) @ np.asarray(M, np.float64))


def seeded_views(grid, extent, seed, n=8):
    """test_gpu_view.seeded_views without the four poses: rotations, scales 0.3 .. 5 (view pixels per level-0 pixel), mild perspective,
    centred somewhere on the content of the extent"""
    rng = np.random.RandomState(seed)
    geo = grid[1]
    ox, oy = extent_origin(grid, extent)
    out = []
    for _ in range(n):
        a = rng.uniform(-np.pi, np.pi); s = 0.3 * (5 / 0.3) ** rng.uniform(0, 1) / geo[5]
        V = np.array([[s * np.cos(a), -s * np.sin(a), 0.0], [s * np.sin(a), s * np.cos(a), 0.0], [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])
        c = np.array([ox + rng.uniform(0.2, 0.8) * extent[2] * geo[4], oy + rng.uniform(0.2, 0.8) * extent[3] * geo[4], 1.0])
        p = V @ c
        V[0, 2] = rng.uniform(10, 60) * p[2] - p[0]; V[1, 2] = rng.uniform(2, 30) * p[2] - p[1]
        out.append(V)
    return out


def level_crops(extent, k):
    """(ax, ay, width, height) in level-k pixels for the shape `holes` (5 x 3 slots; the hole at (2, 2) of the extent, column 3 absent
    but for nothing, column 4 held by one tile): a crop that starts on a tile border, one that ends on one, one over the hole, the
    absent column and their neighbours, two that leave the extent at opposite corners, one wholly outside.  At most 200 x 60."""
    e = ELE >> k
    cols, rows = extent[2] * e, extent[3] * e
    w, h = min(200, 2 * e + 5), min(60, e + 3)
    w2, h2 = min(150, 2 * e), min(60, e)
    return ((e, e, w, h), (3 * e - w2, 2 * e - h2, w2, h2), (3 * e - w // 2, 2 * e - h // 2, w, h),
            (-(w // 3) - 1, -(h // 3) - 1, w, h), (cols - w // 2, rows - h // 2, w, h), (cols + 5, 3, 64, 48))


def crop_of_truth(S, Cv, ax, ay, w, h, channels=4):
    """what a crop at scale 1 is outright: the pixels of S_k and C_k, the background with coverage 0 outside the extent"""
    want = np.zeros((h, w, 4), np.uint8); want[:, :, :3] = pi.BG
    rows, cols = Cv.shape
    x0, y0, x1, y1 = max(ax, 0), max(ay, 0), min(ax + w, cols), min(ay + h, rows)
    inside = x0 < x1 and y0 < y1
    if inside:
        want[y0 - ay:y1 - ay, x0 - ax:x1 - ax, :3] = S[y0:y1, x0:x1]
        want[y0 - ay:y1 - ay, x0 - ax:x1 - ax, 3] = Cv[y0:y1, x0:x1]
    return want[:, :, :channels], inside


# ---------------------------------------------------------------- the lone pixels under sub-pixel shifts
LONE_SEED = 4                                     # the first tile's lone pixel is pi.LONE[4] = (7, 31): inside the tile, far from any other
LONE_SHIFTS = [(a, b) for b in (0, 1, 2, 16, 31) for a in (0, 1, 2, 3, 16, 30, 31)]
LONE_SIZE = (7, 6)


def lone_pixel(m):
    """(column, row) in the extent of the lone pixel of the model's first tile at level 0"""
    t = next(iter(m.tiles_))                      # make_tiles' first coordinate: its lone position is pi.LONE[seed % 10]
    assert m.w_kinds[t] in ("lone_one", "lone_zero")
    w0 = m.tiles_[t][1][0]
    at = np.argwhere(w0 != 0) if m.w_kinds[t] == "lone_one" else np.argwhere(w0 == 0)
    assert len(at) == 1
    ex = extent_of(m.tiles())
    return (t[0] - ex[0]) * ELE + int(at[0][1]), (t[1] - ex[1]) * ELE + int(at[0][0])


def lone_view(grid, m, a, b):
    """scale 1 at level 0, shifted by (a / 32, b / 32): view pixel (3, 3) lies a / 32, b / 32 behind the lone pixel, which is its first
    tap; view pixel (2, 2) has it as its last tap, with the weight a b 32 of 32768"""
    px, py = lone_pixel(m)
    return crop_view(grid, extent_of(m.tiles()), 0, px - 3 + a / 32.0, py - 3 + b / 32.0)


# ---------------------------------------------------------------- far coordinates
def far_views(grid, extent):
    """{name: V} of 64 x 48 views over an extent of 3 x 3 tiles whose source coordinates leave the ranges the warp converts through:
    `short`  a pitch of 3000 level-0 pixels: beyond a few view pixels sx = X >> 5 leaves the short range (sat_short);
    `int`    a pitch of 2e6 level-0 pixels: 32 x passes 2^31 on the right and below (the convert to int saturates), not on the left;
    `fivefold`  a perspective whose denominator runs from 1 to 5 along a row and keeps its sign.
    Each puts the content under interior view pixels: (30, 20), (10, 8), and columns 10 and up."""
    views = {}
    for name, pitch, (u, v) in (("short", 3000.0, (30, 20)), ("int", 2.0e6, (10, 8))):
        views[name] = pixel_view(grid, extent, [[pitch, 0, 300.3 - u * pitch], [0, pitch, 400.6 - v * pitch], [0, 0, 1.0]])
    views["fivefold"] = pixel_view(grid, extent, [[42.6, 0, -200.0], [0, 40.0, -300.0], [4.0 / 63, 0, 1.0]])
    return views


# ---------------------------------------------------------------- the weight cases of tests/test_gpu_view_inject.py
WEIGHT_KINDS = ("signs", "nonfinite", "lone_one", "lone_zero", "none", "all")
WEIGHT_VIEW_SEED = 25                             # its first two views lie over four tiles each, not over the hole or the absent column


def weight_map_args(force_float, w_kind):
    """5 bands on the map with holes, the colour kind `view`; the seeds of the two types five apart, as in tests/test_gpu_inject.py"""
    return (5, force_float, "holes", "view", w_kind, 7 + 5 * force_float)


def weight_views(grid, m):
    """[(level asked, V, width, height, crop)]: level_crops at every level k, asked at level k and at -1, crop = (k, ax, ay); and two
    general homographies at every explicit level and at -1, crop = None"""
    ex = extent_of(m.tiles())
    out = []
    for k in range(m.num_levels):
        for c in level_crops(ex, k):
            V = crop_view(grid, ex, k, c[0], c[1])
            out += [(k, V, c[2], c[3], (k, c[0], c[1])), (-1, V, c[2], c[3], (k, c[0], c[1]))]
    for V in seeded_views(grid, ex, WEIGHT_VIEW_SEED, 2):
        out += [(level, V, 150, 37, None) for level in [-1] + list(range(m.num_levels))]
    return out
