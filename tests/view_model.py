"""The model of a rendered view (pf_render_view*, DESIGN.md "Views"), test code only.

A view is cv::warpPerspective of the 4-channel image B G R C -- the mosaic S_k at pyramid level k and its coverage C_k, cropped to the
plan's rectangle of tiles -- by the plan's M0, then bg_color under coverage 0.  The warp is the oracle's orc.warp_linear_const_8u; this
module restates none of its arithmetic: it crops, stacks, calls and paints."""
import numpy as np

from oracle import orc

ELE = 256


def view_model(S, C, origin, info, width, height, bg, channels=4):
    """S: the mosaic at level info["level"] (rows x cols x 3 uint8), C: its coverage (rows x cols, 0 / 255), origin: the mosaic's first
    tile (stable tile coordinates), info: the plan (pf_view_plan / render_view's dict).  S, C may be None for a map without content."""
    paint = np.uint8(min(max(bg, 0), 255))
    if info["empty"]:
        out = np.zeros((height, width, 4), np.uint8)
        out[:, :, :3] = paint
        return out[:, :, :channels].copy()
    e = ELE >> info["level"]
    tx, ty, nx, ny = info["rect"]
    x0, y0 = (tx - origin[0]) * e, (ty - origin[1]) * e
    assert 0 <= x0 and 0 <= y0 and x0 + nx * e <= S.shape[1] and y0 + ny * e <= S.shape[0], "the rectangle leaves the extent"
    src = np.concatenate([S[y0:y0 + ny * e, x0:x0 + nx * e], C[y0:y0 + ny * e, x0:x0 + nx * e, None]], axis=2)
    out = orc.warp_linear_const_8u(np.ascontiguousarray(src), np.asarray(info["M0"], np.float64).reshape(3, 3), height, width)
    out[out[:, :, 3] == 0, :3] = paint
    return out[:, :, :channels].copy()


def coverage_of(weights_k):
    """C_k of a level-k weight plane: 255 where the weight is not 0"""
    return np.where(weights_k != 0, 255, 0).astype(np.uint8)


# ---------------------------------------------------------------- the rig of the view tests: small maps that reach every rule
CAM = [160, 120, 125, 125, 80, 60]
ROWS, COLS = 120, 160
BG = 201
STEP = (100.0, 60.0)                     # about half a tile a keyframe: 8 keyframes give 5 x 4 tiles
_ORACLES, _TRUTH = {}, {}


def rig_poses(n=8, seed=4):
    from helpers import jitter_poses
    return jitter_poses(n, seed=seed, step=STEP)


def rig_frame(k):
    from helpers import HOSTILE_KINDS, hostile_frame
    return hostile_frame(("noise", "ramp", "checker2", "noise", "step", "noise", "impulse", "noise", "ramp", "noise")[k % 10], ROWS, COLS, k)


def oracle_map(force_float, bands, upto=8, n=8, seed=4, prep=None):
    """The oracle fed the first `upto` of the rig's n keyframes (prepared from poses[:prep], all of them by default).  Cached and shared:
    the tests must not feed it."""
    from helpers import workloads
    key = (force_float, bands, upto, n, seed, prep)
    if key not in _ORACLES:
        poses = rig_poses(n, seed)
        o = orc.OracleMap(band_num=bands, force_float=force_float, bg_color=BG)
        assert o.prepare(workloads().IDENTITY_PLANE, CAM, poses[:prep] if prep else poses)
        for k in range(upto):
            assert o.feed(rig_frame(k), poses[k])
        _ORACLES[key] = o
    return _ORACLES[key]


def extent_of(tiles):
    xs, ys = [t[0] for t in tiles], [t[1] for t in tiles]
    return (min(xs), min(ys), max(xs) + 1 - min(xs), max(ys) + 1 - min(ys))


def truth(o, k):
    """(S_k, C_k, origin) of an oracle map: level 0 is the oracle's own save(), level k > 0 level_view_model's model_save_level of the
    oracle's tiles; the coverage is the oracle's level-k weights pasted over the extent.  Cached by map and level and left unchanged."""
    from types import SimpleNamespace
    from level_view_model import model_save_level
    key = (id(o), k)
    if key not in _TRUTH:
        tiles = o.tiles()
        L = o.num_levels - 1
        x0, y0, nx, ny = extent_of(tiles)
        e = ELE >> k
        wk = np.zeros((ny * e, nx * e), np.float32)
        held = {}
        for t in tiles:
            lv = [o.tile_level(t[0], t[1], i) for i in range(L + 1)]
            held[t] = ([a[0] for a in lv], [a[1] for a in lv])
            wk[(t[1] - y0) * e:(t[1] - y0 + 1) * e, (t[0] - x0) * e:(t[0] - x0 + 1) * e] = lv[k][1]
        if k == 0:
            S, origin = o.save()
        else:
            S, origin = model_save_level(SimpleNamespace(tiles_=held, L=L, dtype=o.dtype, bg_color=BG), k)
        assert origin == (x0, y0) and S.shape[:2] == wk.shape
        _TRUTH[key] = (S, coverage_of(wk), origin, held)
    return _TRUTH[key][:3]


def held_tiles(o):
    truth(o, 0)
    return _TRUTH[(id(o), 0)][3]
