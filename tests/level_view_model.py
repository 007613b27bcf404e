"""The reduced-resolution views of a ModelMap (map_model.py): the pyramid collapsed from the top and stopped at level k, test code only.

The blending rule is self-similar -- Ele::blend's halo at level i is 1 << (nl-1-i) -- so the view of level k is Ele::blend / save() of
a map whose tiles are 256 >> k pixels wide with levels k .. L.  Written from map_model's primitives (pyr_up, _sat16, to_8u) with the
square assembly of ModelMap._blend and the paste of ModelMap._save restated for levels k .. L; shares no code with the HIP library."""
import numpy as np

from map_model import ELE, _sat16, pyr_up, to_8u


def collapse_from(levels, k):
    """restoreImageFromLaplacePyr stopped at level k: from the top, G_{i-1} = pyrUp(G_i) + L_{i-1} (saturating add for 16S) down to
    G_k.  k = len(levels) - 1 returns the top level itself."""
    g = levels[-1]
    for i in range(len(levels) - 2, k - 1, -1):
        up = pyr_up(g)
        if up.dtype == np.float32:
            g = up + levels[i]
        else:
            g = _sat16(up.astype(np.int64) + levels[i].astype(np.int64))
    return g


def model_blend_level(m, ix, iy, k):
    """Ele::blend truncated at level k, raw (the pyramid type), E x E x 3 with E = 256 >> k: the padded squares of levels k .. L with
    their halos of 1 << (L - i) when all nine tiles are there and high_quality is on, cropped at 1 << (L - k); otherwise the tile's
    own levels k .. L.  Pixels whose LEVEL-k weight is 0 are 0.  None for a tile that does not exist."""
    t = m.tiles_.get((ix, iy))
    if t is None:
        return None
    L, e = m.L, ELE >> k
    nb = [m.tiles_.get((ix + dx, iy + dy)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if m.high_quality and all(n is not None for n in nb):
        lv = [None] * k
        for i in range(k, L + 1):
            b, s = 1 << (L - i), ELE >> i
            big = np.empty((s + 2 * b, s + 2 * b, 3), m.dtype)
            for yy in range(3):
                for xx in range(3):
                    src = nb[3 * yy + xx][0][i]
                    rs = slice(s - b, s) if yy == 0 else (slice(0, s) if yy == 1 else slice(0, b))
                    cs = slice(s - b, s) if xx == 0 else (slice(0, s) if xx == 1 else slice(0, b))
                    rd = slice(0, b) if yy == 0 else (slice(b, b + s) if yy == 1 else slice(b + s, s + 2 * b))
                    cd = slice(0, b) if xx == 0 else (slice(b, b + s) if xx == 1 else slice(b + s, s + 2 * b))
                    big[rd, cd] = src[rs, cs]
            lv.append(big)
        bk = 1 << (L - k)
        out = collapse_from(lv, k)[bk:bk + e, bk:bk + e].copy()
    else:
        out = collapse_from([a.copy() for a in t[0]], k).copy()
    out[t[1][k] == 0] = 0
    return out


def model_save_level(m, k):
    """save() truncated at level k: levels k .. L of the tiles pasted over their bounding box (absent tiles zero), one collapse down
    to level k, the 8U view, bg_color where the pasted level-k weight is 0.  Returns (image, (tile x0, tile y0)), or None."""
    if not m.tiles_:
        return None
    xs = [t[0] for t in m.tiles_]; ys = [t[1] for t in m.tiles_]
    x0, y0 = min(xs), min(ys)
    wx, wy = max(xs) + 1 - x0, max(ys) + 1 - y0
    e = ELE >> k
    lv = [None] * k + [np.zeros((wy * (ELE >> i), wx * (ELE >> i), 3), m.dtype) for i in range(k, m.L + 1)]
    wk = np.zeros((wy * e, wx * e), np.float32)
    for (ix, iy), (lap, wts) in m.tiles_.items():
        for i in range(k, m.L + 1):
            s = ELE >> i
            lv[i][(iy - y0) * s:(iy - y0 + 1) * s, (ix - x0) * s:(ix - x0 + 1) * s] = lap[i]
        wk[(iy - y0) * e:(iy - y0 + 1) * e, (ix - x0) * e:(ix - x0 + 1) * e] = wts[k]
    out = to_8u(collapse_from(lv, k))
    out[wk == 0] = np.uint8(min(max(m.bg_color, 0), 255))
    return out, (x0, y0)


# ---------------------------------------------------------------- the rig of the level-view tests
def lattice_model(force_float, bands, keep=(0, 1, 2, 3), high_quality=1):
    """The rig of test_gpu_model.py -- camera 333 x 257, the 2 x 2 LATTICE, keyframes of the MIXED hostile kinds, jittered poses,
    bg_color 201 -- with the keyframes `keep` (indices into the lattice, in feed order) fed to a ModelMap; the oracle supplies the
    geometry of each feed, as everywhere (helpers.feed_with_model).  Returns (poses, prep, frames, model): the poses and frames
    of `keep`, the poses the grid is prepared from.  Cached: the tests share the models and must not feed them."""
    key = (force_float, bands, tuple(keep), high_quality)
    if key not in _RIGS:
        from helpers import feed_with_model, hostile_frame, workloads
        from oracle import orc
        from test_gpu_model import BG, CAM, COLS, MIXED, ROWS, lattice_poses
        from map_model import ModelMap
        all_poses = lattice_poses(11 + bands)
        prep = all_poses[:2]
        o = orc.OracleMap(band_num=bands, force_float=force_float, bg_color=BG)
        m = ModelMap(band_num=bands, force_float=force_float, bg_color=BG, high_quality=high_quality)
        assert o.prepare(workloads().IDENTITY_PLANE, CAM, prep)
        poses, frames = [all_poses[k] for k in keep], [hostile_frame(MIXED[k], ROWS, COLS, k) for k in keep]
        for f, p in zip(frames, poses):
            assert feed_with_model(o, m, f, p)
        _RIGS[key] = (poses, prep, frames, m)
    return _RIGS[key]


_RIGS = {}
