"""Pyramids put straight into a map's tile slots (pf_tile_import) and into ModelMap.tiles_ alike, test code only: the output side --
Ele::blend, the 8U view, save, the level-k views, the coverage masks, the halo strips -- on stored state that no keyframe would leave
behind.  The slot layout is restated here from its rule, the contents come from seeded generators, one stream per tile and level.

Nothing here needs a GPU to import; build() does."""
import numpy as np

ELE = 256
PAD = 0xA5                                   # what pack() leaves in the alignment padding of a slot: nothing may need it to be zero
BG = 201
RAILS = (-32768, -32767, -1, 0, 1, 32766, 32767)
LONE = ((0, 0), (0, 255), (255, 0), (255, 255), (7, 31), (8, 32), (31, 3), (32, 4), (63, 127), (64, 128))
LAP_KINDS = {0: ("rails", "full", "opposed", "view"), 1: ("view", "wide", "big", "ties")}
W_KINDS = ("half", "all", "none", "lone_one", "lone_zero", "signs")
SHAPES = {
    "one": [(-3, 2)],
    "nine": [(x, y) for y in (-2, -1, 0) for x in (-1, 0, 1)],                                  # the centre (0, -1) has all nine
    "holes": [(x, y) for y in (1, 2, 3) for x in (-2, -1, 0) if (x, y) != (0, 3)] + [(2, 2)],   # 5 x 3 slots, 9 tiles, none with nine
    "row": [(x, -1) for x in (-2, -1, 0, 1, 2)],
    "column": [(3, y) for y in (-3, -2, -1, 0)],
}


# ---------------------------------------------------------------- the slot
def _round256(n):
    return (n + 255) // 256 * 256


def slot_layout(bands, force_float):
    """The tile slot of a multi-band map: nlev = min(bands, 8) + 1 levels; the Laplacians of levels 0 .. L first, (256 >> i)^2 pixels
    of 3 components of 2 (16S) or 4 (32F) bytes each, every level rounded up to 256 bytes; then the weights of levels 0 .. L,
    (256 >> i)^2 floats, rounded up alike.  Returns {"nlev", "lap_off", "w_off", "total"}."""
    nlev = min(max(bands, 0), 8) + 1
    es = 4 if force_float else 2
    off, lap_off, w_off = 0, [], []
    for i in range(nlev):
        lap_off.append(off)
        off += _round256((ELE >> i) ** 2 * 3 * es)
    for i in range(nlev):
        w_off.append(off)
        off += _round256((ELE >> i) ** 2 * 4)
    return {"nlev": nlev, "lap_off": lap_off, "w_off": w_off, "total": off}


def pack(lap, w, pad=PAD):
    """[lap_0 .. lap_L] (s x s x 3, int16 or float32) and [w_0 .. w_L] (s x s float32) -> the slot's bytes, padding = pad (0xA5)"""
    ff = lap[0].dtype == np.float32
    lay = slot_layout(len(lap) - 1, ff)
    assert len(lap) == len(w) == lay["nlev"]
    out = np.full(lay["total"], pad, np.uint8)
    for i in range(lay["nlev"]):
        s = ELE >> i
        assert lap[i].shape == (s, s, 3) and lap[i].dtype == (np.float32 if ff else np.int16) and w[i].shape == (s, s) and w[i].dtype == np.float32
        a, b = np.ascontiguousarray(lap[i]).view(np.uint8).reshape(-1), np.ascontiguousarray(w[i]).view(np.uint8).reshape(-1)
        out[lay["lap_off"][i]:lay["lap_off"][i] + a.size] = a
        out[lay["w_off"][i]:lay["w_off"][i] + b.size] = b
    return out


def unpack(buf, bands, force_float):
    """the inverse of pack: (lap, w) as copies"""
    lay = slot_layout(bands, force_float)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    assert buf.size == lay["total"]
    dt = np.float32 if force_float else np.int16
    lap, w = [], []
    for i in range(lay["nlev"]):
        s = ELE >> i
        n = s * s * 3 * np.dtype(dt).itemsize
        lap.append(buf[lay["lap_off"][i]:lay["lap_off"][i] + n].copy().view(dt).reshape(s, s, 3))
        w.append(buf[lay["w_off"][i]:lay["w_off"][i] + s * s * 4].copy().view(np.float32).reshape(s, s))
    return lap, w


def padding_of(buf, bands, force_float):
    """the bytes of a slot image that belong to no level"""
    lay = slot_layout(bands, force_float)
    used = np.zeros(lay["total"], bool)
    es = 4 if force_float else 2
    for i in range(lay["nlev"]):
        n = (ELE >> i) ** 2
        used[lay["lap_off"][i]:lay["lap_off"][i] + n * 3 * es] = True
        used[lay["w_off"][i]:lay["w_off"][i] + n * 4] = True
    return np.asarray(buf, np.uint8).reshape(-1)[~used]


# ---------------------------------------------------------------- Laplacian contents
def _tie_table():
    """{n: float32 v with float32(v) * float32(255) == n + 0.5 exactly} for n = -2 .. 257, searched among float32((n + .5) / 255) and
    its neighbours.  The product is the fp32 8U view's argument: these are the values at which its rounding is a tie."""
    out = {}
    for n in range(-2, 258):
        t = np.float32(n + 0.5)
        v0 = np.float32((n + 0.5) / 255.0)
        cands = [v0]
        lo = hi = v0
        for _ in range(8):
            lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
            cands += [lo, hi]
        hit = [v for v in cands if np.float32(v) * np.float32(255) == t]
        assert hit, "no float32 v with v * 255 == %g" % t
        out[n] = hit[0]
    return out


_TIES = None


def tie_values():
    global _TIES
    if _TIES is None:
        _TIES = _tie_table()
    return _TIES


def _finite_band(a):
    """fp32 contents stay finite and, unless 0, within [2^-60, 2^60]: the collapse kernels' carried odd sum is exact only without
    overflow or underflow"""
    a = a.astype(np.float32)
    a[np.abs(a) < np.float32(2.0 ** -60)] = 0
    assert np.isfinite(a).all() and np.abs(a).max() <= 2.0 ** 60
    return a


def opposed_value(i, L):
    """The `opposed` pyramid: every level constant (pyrUp of a constant is that constant, at every border form), level L +32767, below
    it -32768 / +32767 in runs of two levels counted from level 0 (levels 0, 1: -32768; 2, 3: +32767; ...).  Alternating level by
    level never saturates -- the collapse walks 32767, -1, 32766, -2, ... -- while two equal rails in a row do: from about 0 the
    first lands next to a rail and the second goes over it.  At 5 bands: 32767, -1, 32766, [32767], -1, [-32768]; at 8 bands both
    directions as well.  Every pixel alike."""
    if i == L:
        return 32767
    return -32768 if (i // 2) % 2 == 0 else 32767


def make_lap(kind, force_float, L, rng):
    """[lap_0 .. lap_L] of one tile; rng is the tile's own generator, the levels drawn one after the other"""
    out = []
    for i in range(L + 1):
        s = ELE >> i
        shp = (s, s, 3)
        if not force_float:
            if kind == "rails":
                a = np.asarray(RAILS, np.int16)[rng.integers(0, len(RAILS), shp)]
            elif kind == "full":
                a = rng.integers(-32768, 32768, shp).astype(np.int16)
            elif kind == "opposed":
                a = np.full(shp, opposed_value(i, L), np.int16)
            elif kind == "view":
                a = (rng.integers(0, 256, shp) if i == 0 else rng.integers(-40, 41, shp)).astype(np.int16)
            else:
                raise ValueError(kind)
        else:
            if kind == "view":
                a = _finite_band(rng.uniform(0, 1, shp) if i == 0 else rng.uniform(-0.1, 0.1, shp))
            elif kind == "wide":
                a = _finite_band(rng.uniform(-2, 3, shp))
            elif kind == "big":
                a = _finite_band(1e4 * rng.integers(-3, 4, shp))               # steps of +-1e4 between neighbours, up to +-6e4
            elif kind == "ties":
                if i == 0:
                    tab = tie_values()
                    vals = np.array([tab[n] for n in range(-2, 258)], np.float32)
                    a = vals[rng.integers(0, vals.size, shp)]
                else:
                    a = np.zeros(shp, np.float32)
            else:
                raise ValueError(kind)
        out.append(np.ascontiguousarray(a))
    return out


# ---------------------------------------------------------------- weight contents
def lone_positions(level):
    """LONE scaled into the level, without duplicates, in LONE's order"""
    out = []
    for r, c in LONE:
        p = (r >> level, c >> level)
        if p not in out:
            out.append(p)
    return out


def _positive(rng, shp):
    return rng.uniform(0.01, 1.0, shp).astype(np.float32)


def make_w(kind, L, rng, pos=0):
    """[w_0 .. w_L] of one tile.  pos: which entry of lone_positions() a lone_* tile uses (modulo their number at each level)."""
    out = []
    for i in range(L + 1):
        s = ELE >> i
        shp = (s, s)
        if kind == "half":
            a = _positive(rng, shp)
            a[rng.random(shp) < 0.5] = 0
        elif kind == "all":
            a = _positive(rng, shp)
        elif kind == "none":
            a = np.zeros(shp, np.float32)
        elif kind in ("lone_one", "lone_zero"):
            ps = lone_positions(i)
            p = ps[pos % len(ps)]
            if kind == "lone_one":
                a = np.zeros(shp, np.float32); a[p] = _positive(rng, (1,))[0]
            else:
                a = _positive(rng, shp); a[p] = 0
        elif kind == "signs":
            # -0.0 is zero; the denormals, FLT_MIN, negative normals and positives are not (IEEE w != 0)
            pool = np.array([-0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, -0.75, -3e-30, 0.5, 2e-20], np.float32)
            a = pool[rng.integers(0, pool.size, shp)]
            neg = rng.random(shp) < 0.125
            a[neg] = -_positive(rng, shp)[neg]                                  # negative normals of any mantissa
        else:
            raise ValueError(kind)
        out.append(np.ascontiguousarray(a, dtype=np.float32))
    return out


# ---------------------------------------------------------------- whole maps
def make_tiles(bands, force_float, shape, lap_kind, w_kind, seed):
    """{(ix, iy): ([lap_0 .. lap_L], [w_0 .. w_L])} over SHAPES[shape] (or a list of coordinates) and {(ix, iy): weight kind}.  With a
    weight kind other than "half", every second tile (the first, third, ...) is of that kind and the others are "half": the shared
    all-zero / all-one mask tiles then lie beside tiles of their own, and a blend's neighbours differ from it."""
    L = min(max(bands, 0), 8)
    coords = SHAPES[shape] if isinstance(shape, str) else list(shape)
    assert len(coords) <= 10
    tiles, kinds = {}, {}
    for j, t in enumerate(coords):
        rng = np.random.default_rng([seed, j, bands, int(bool(force_float))])
        wk = w_kind if (w_kind == "half" or j % 2 == 0) else "half"
        tiles[t] = (make_lap(lap_kind, force_float, L, rng), make_w(wk, L, rng, pos=seed + j // 2))
        kinds[t] = wk
    return tiles, kinds


def model_of(tiles, bands, force_float, high_quality=1, bg=BG):
    from map_model import ModelMap
    m = ModelMap(band_num=bands, force_float=force_float, bg_color=bg, high_quality=high_quality)
    m.tiles_ = {t: ([a.copy() for a in lw[0]], [a.copy() for a in lw[1]]) for t, lw in tiles.items()}
    return m


def import_tiles(g, tiles):
    """every tile through a torch uint8 CUDA tensor into the map (pf_tile_import); returns the packed slot images by coordinate"""
    import torch
    packed = {}
    for t, (lap, w) in tiles.items():
        packed[t] = pack(lap, w)
        dev = torch.from_numpy(packed[t]).cuda()
        torch.cuda.synchronize()
        assert g.tile_import(t[0], t[1], dev.data_ptr()), t
        del dev
    return packed


def new_map(pf, bands, force_float, **opt):
    """an empty TypeMultiBandCPU map (thread = False), prepared as tests/test_gpu_model.py prepares its maps: tile_import needs a
    prepared map"""
    from helpers import workloads
    from test_gpu_model import CAM, lattice_poses
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, band_number=bands, bg_color=BG, **opt)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, lattice_poses(11 + bands)[:2])
    return g


def build(pf, bands, force_float, shape, lap_kind, w_kind, seed, **opt):
    """new_map with the tiles of make_tiles imported -- the extent of a save comes from the tile store, not from the grid -- and a
    ModelMap whose tiles_ holds the same arrays.  Returns (map, model); the model carries .packed and .w_kinds by tile coordinate."""
    tiles, kinds = make_tiles(bands, force_float, shape, lap_kind, w_kind, seed)
    g = new_map(pf, bands, force_float, **opt)
    m = model_of(tiles, bands, force_float, opt.get("high_quality_show", 1))
    m.packed = import_tiles(g, tiles)
    m.w_kinds = kinds
    return g, m
