"""The output-side kernels on stored state that no keyframe leaves behind (pyramid_inject.py): k_collapse_fused (Ele::blend, the 8U view,
save), k_collapse_level (the views of level k), k_coverage_tiles / k_coverage_expand (the masks of the masked TIFF) and the halo-strip
path (halo_pack, fetch_blend with strip_mask), against ModelMap / level_view_model on the very arrays that were imported.  Pinned here
and nowhere else: the saturation of the 16S restore (full-range Laplacians), the IEEE zero test of the weights at every level (lone
pixels, -0.0, denormals, whole tiles of zeros), ties to even in the fp32 8U view, clipped blocks of the level mosaics (maps one tile
wide or high), strips at 1, 5 and 8 bands.  Every comparison is exact."""
import numpy as np
import pytest

import pyramid_inject as pi
import tiff_mask_model as mm
import tiff_model as tm
from level_view_model import model_blend_level, model_save_level
from map_model import canvas_geometry, to_8u
from test_gpu_level_view import ABSENT, SENTINEL, shuffled
from test_gpu_tiff import transform_of
from test_gpu_tiff_mask import host_masked
from test_tiff import encoder

pytestmark = pytest.mark.gpu

BG = pi.BG
NINE_KINDS = [(ff, kind) for ff in (0, 1) for kind in pi.LAP_KINDS[ff]]
FULL = {0: "full", 1: "wide"}


def same_bytes(a, b):
    """equal bit for bit: tells -0.0 from 0.0, which np.array_equal does not"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_layout(g, m, bands, ff):
    import torch
    lay = pi.slot_layout(bands, ff)
    assert g.tile_bytes() == lay["total"] and g.num_levels == m.num_levels == lay["nlev"]
    assert g.tiles() == m.tiles()
    buf = torch.full((lay["total"] + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                             # the map works on a stream of its own: the fill comes first
    for t in m.tiles():
        for i in range(m.num_levels):
            gl, gw = g.tile_level(*t, i)
            ml, mw = m.tile_level(*t, i)
            assert same_bytes(gl, ml) and same_bytes(gw, mw), (t, i)
        assert g.tile_export(t[0], t[1], buf.data_ptr())
        got = buf.cpu().numpy()
        assert np.array_equal(got[:lay["total"]], m.packed[t]) and (got[lay["total"]:] == 0x5A).all(), t          # padding included
    changed, px = g.blend_changed(cap=16)
    assert sorted(changed) == sorted(m.tiles()) and len(changed) == len(m.tiles())          # exactly the imported tiles, once
    for t, im in zip(changed, px):
        assert np.array_equal(im, m.blend_tile(*t)), ("blend_changed", t)
    assert g.blend_changed(cap=16)[0] == []


def check_views(g, m, shape):
    """levels 0 .. L: the tile views, raw and 8U, in a shuffled order around a coordinate without a tile, and the mosaic"""
    clipped = False
    for k in range(m.num_levels):
        e = 256 >> k
        order = shuffled(m.tiles(), 17 + k)
        raw = np.empty((len(order), e, e, 3), m.dtype)
        raw.view(np.uint8)[:] = SENTINEL
        sentinel_raw = raw[0].copy()
        bgr = np.full((len(order), e, e, 3), SENTINEL, np.uint8)
        assert g.blend_tiles_raw(order, level=k, out=raw) is not None
        assert g.blend_tiles(order, out=bgr, level=k) is not None
        for i, t in enumerate(order):
            if t == ABSENT:
                assert (bgr[i] == SENTINEL).all() and raw[i].tobytes() == sentinel_raw.tobytes(), (k, "absent tile written")
                continue
            want = m.blend_tile_raw(*t) if k == 0 else model_blend_level(m, *t, k)
            assert np.array_equal(raw[i], want), (k, t, "raw", int((raw[i] != want).sum()))
            assert np.array_equal(bgr[i], to_8u(want)), (k, t, "8U", int((bgr[i] != to_8u(want)).sum()))
            if k == 0:
                assert np.array_equal(g.blend_tile_raw(*t), want), (t, "blend_tile_raw")
        got, origin = g.save_to_memory(level=k)
        want, want_origin = m.save() if k == 0 else model_save_level(m, k)
        assert origin == want_origin and got.shape == want.shape, k
        assert np.array_equal(got, want), (k, "mosaic", int((got != want).any(axis=2).sum()))
        if k and (got.shape[1] % 128 or got.shape[0] % 32):
            clipped = True
    if shape in ("row", "column") and m.num_levels > 3:
        assert clipped                                                   # blocks clipped to the mosaic ran (bw = colsk - X0, bh = rowsk - Y0)


def pasted_mask(m, shape2, org):
    want = np.zeros(shape2, np.uint8)
    for (ix, iy), (_, w) in m.tiles_.items():
        want[(iy - org[1]) * 256:(iy - org[1] + 1) * 256, (ix - org[0]) * 256:(ix - org[0] + 1) * 256] = (w[0] != 0) * 255
    return want


def check_masks_and_tiff(pf, g, m, tmp_path):
    ref, ref_org = m.save()
    mem, mask, org = g.save_to_memory_mask()
    assert org == ref_org and np.array_equal(mem, ref)
    want = pasted_mask(m, mem.shape[:2], org)
    assert np.array_equal(mask, want), int((mask != want).sum())
    assert (mem[mask == 0] == BG).all()
    xf = transform_of(g, org)
    f = str(tmp_path / "m.tif")
    assert g.save_tiff_masked(f)
    data = open(f, "rb").read()
    assert data == host_masked(pf, str(tmp_path / "h.tif"), mem, mask, 95, BG, xf)
    mm.check_masked_file(data, mem, mask, BG, encoder(pf, 95), xf)
    # the level-0 mask tile of every slot: shared all-zero (no tile, or a tile of zero weights), shared all-one, or one of its own
    _, ifds = tm.parse(data)
    lv0 = ifds[1]["tags"][324][1]
    tx = mem.shape[1] // 256
    masks = mm.mask_chain(mask)
    shared = {kd: {o for ifd, mk in zip(ifds[1::2], masks) for o, t in zip(ifd["tags"][324][1], mm.mask_tiles_of(mk)) if mm.kind_of(t) == kd}
              for kd in ("zero", "one")}
    assert len(shared["zero"]) <= 1 and len(shared["one"]) <= 1
    for y in range(mem.shape[0] // 256):
        for x in range(tx):
            kind = m.w_kinds.get((x + org[0], y + org[1]), "absent")
            off = lv0[y * tx + x]
            if kind in ("absent", "none"):
                assert off in shared["zero"], (x, y, kind)
            elif kind == "all":
                assert off in shared["one"], (x, y, kind)
            else:
                assert off not in shared["zero"] | shared["one"] and lv0.count(off) == 1, (x, y, kind)


def check_map(pf, tmp_path, bands, ff, shape, lap_kind, w_kind, seed, **opt):
    g, m = pi.build(pf, bands, ff, shape, lap_kind, w_kind, seed, **opt)
    check_layout(g, m, bands, ff)
    check_views(g, m, shape)
    check_masks_and_tiff(pf, g, m, tmp_path)
    g.close()


@pytest.mark.parametrize("ff,kind", NINE_KINDS)
def test_every_laplacian_kind_on_nine_tiles(pf, tmp_path, ff, kind):
    """5 bands; the centre takes the bordered branch of Ele::blend, the rim blends alone"""
    check_map(pf, tmp_path, 5, ff, "nine", kind, "half", 1)


@pytest.mark.parametrize("shape", list(pi.SHAPES))
@pytest.mark.parametrize("bands", [1, 8])
@pytest.mark.parametrize("ff", [0, 1])
def test_every_shape_at_one_and_eight_bands(pf, tmp_path, ff, bands, shape):
    check_map(pf, tmp_path, bands, ff, shape, FULL[ff], "half", 2)


@pytest.mark.parametrize("bands", [0, 2])
@pytest.mark.parametrize("ff", [0, 1])
def test_zero_and_two_bands(pf, tmp_path, ff, bands):
    check_map(pf, tmp_path, bands, ff, "nine", FULL[ff], "half", 3)


@pytest.mark.parametrize("w_kind", pi.W_KINDS)
@pytest.mark.parametrize("ff", [0, 1])
def test_every_weight_kind_on_a_map_with_holes(pf, tmp_path, ff, w_kind):
    """5 bands; the seeds of the two types are five apart: their lone pixels cover all ten positions"""
    check_map(pf, tmp_path, 5, ff, "holes", FULL[ff], w_kind, 7 + 5 * ff)


@pytest.mark.parametrize("ff", [0, 1])
def test_without_high_quality_show_every_tile_blends_alone(pf, tmp_path, ff):
    check_map(pf, tmp_path, 5, ff, "nine", FULL[ff], "half", 4, high_quality_show=0)


# ---------------------------------------------------------------- halo strips
def strip_of(lap, dx, dy, nlev):
    """what halo_pack(ix, iy, dx, dy) packs of a tile that is the (dx, dy) neighbour of the one blended: of every level the edge facing
    it, 1 << (nlev - 1 - i) pixels deep, rows top to bottom, the levels back to back"""
    out = []
    for i, a in enumerate(lap):
        s, b = 256 >> i, 1 << (nlev - 1 - i)
        rs = slice(s - b, s) if dy < 0 else (slice(0, b) if dy > 0 else slice(0, s))
        cs = slice(s - b, s) if dx < 0 else (slice(0, b) if dx > 0 else slice(0, s))
        out.append(np.ascontiguousarray(a[rs, cs]).reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("ff", [0, 1])
def test_halo_strips_stand_in_for_the_neighbours(pf, ff, bands):
    """map A holds nine tiles, map B only the centre: B's blend of it from the eight strips packed out of A is the model's blend of
    A's centre, raw and 8U.  Every strip is packed into a buffer of exactly halo_bytes with guard bytes behind it."""
    import torch
    kind = "wide" if ff else "rails"
    a, m = pi.build(pf, bands, ff, "nine", kind, "half", 6)
    centre = pi.SHAPES["nine"][4]
    b = pi.new_map(pf, bands, ff)
    pi.import_tiles(b, {centre: m.tiles_[centre]})
    assert b.tiles() == [centre]
    nlev = m.num_levels
    halos, keep = [0] * 9, []
    for j, (dx, dy) in enumerate([(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]):
        if (dx, dy) == (0, 0):
            continue
        nb = (centre[0] + dx, centre[1] + dy)
        n = b.halo_bytes(dx, dy)
        want = strip_of(m.tiles_[nb][0], dx, dy, nlev)
        assert n == want.nbytes and n == a.halo_bytes(dx, dy)
        buf = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                         # the map packs on a stream of its own: the fill comes first
        assert a.halo_pack(nb[0], nb[1], dx, dy, buf.data_ptr())
        got = buf.cpu().numpy()
        assert got[:n].tobytes() == want.tobytes() and (got[n:] == 0x5A).all(), (dx, dy)
        keep.append(buf); halos[j] = buf.data_ptr()
    want = m.blend_tile_raw(*centre)
    alone = pi.model_of({centre: m.tiles_[centre]}, bands, ff).blend_tile_raw(*centre)
    assert not np.array_equal(want, alone)                               # the neighbours matter
    assert np.array_equal(b.blend_tile_halo(centre[0], centre[1], halos, raw=True), want)
    assert np.array_equal(b.blend_tile_halo(centre[0], centre[1], halos), to_8u(want))
    assert np.array_equal(b.blend_tile_raw(*centre), alone)              # and without strips B blends it alone
    a.close(); b.close()


# ---------------------------------------------------------------- a keyframe over imported tiles
@pytest.mark.parametrize("ff", [0, 1])
def test_a_keyframe_over_imported_tiles_equals_the_model(pf, orc, ff):
    """Keyframe 0 of test_gpu_model.py's rig is fed (its weight bounds enter the cull), then `view` pyramids are imported over every
    tile keyframe 1 covers -- weights half zero in one, a constant 1e30 in another, all zero or half zero in the rest -- and keyframe 1
    is fed: the import leaves "nothing known" bounds, so no cell may be skipped on the strength of keyframe 0's.  Every level of
    every tile equals the model's select over the imported arrays.
    The select over imported weights -- zeros, a weight nothing beats, `>=` at every level -- is what is pinned here.  With these
    poses no cell of keyframe 1 lies wholly under keyframe 0's bounds: that tile_import forgets the old bounds is pinned by
    tests/test_gpu_feed_slots.py::test_import_forgets_the_cull_bounds, on a rig where the cull bites."""
    from helpers import feed_with_model, hostile_frame, workloads
    from map_model import ModelMap
    from test_gpu_model import CAM, COLS, MIXED, ROWS, lattice_poses
    bands = 5
    poses = lattice_poses(11 + bands)
    prep = poses[:2]
    frames = [hostile_frame(MIXED[k], ROWS, COLS, k) for k in (0, 1)]
    # the tiles keyframe 1 will cover, from a dry run of the geometry
    dry = orc.OracleMap(band_num=bands, force_float=ff, bg_color=BG)
    assert dry.prepare(workloads().IDENTITY_PLANE, CAM, prep) and dry.feed(frames[0], poses[0]) and dry.feed(frames[1], poses[1])
    (offx, offy), (x0, y0, x1, y1), _, _ = canvas_geometry(frames[1].shape, dry.grid(), dry.footprint(poses[1]), dry.last_canvas()[1])
    coords = [(x + offx, y + offy) for y in range(y0, y1) for x in range(x0, x1)]
    assert 2 <= len(coords) <= 10
    tiles = {}
    for j, t in enumerate(coords):
        rng = np.random.default_rng([99, j, ff])
        lap = pi.make_lap("view", ff, bands, rng)
        if j == 1:
            w = [np.full((256 >> i, 256 >> i), 1e30, np.float32) for i in range(bands + 1)]
        else:
            w = pi.make_w("half" if j % 2 == 0 else "none", bands, rng)
        tiles[t] = (lap, w)

    o = orc.OracleMap(band_num=bands, force_float=ff, bg_color=BG)
    m = ModelMap(band_num=bands, force_float=ff, bg_color=BG)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, band_number=bands, bg_color=BG)
    assert o.prepare(workloads().IDENTITY_PLANE, CAM, prep) and g.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    assert feed_with_model(o, m, frames[0], poses[0]) and g.feed(frames[0], poses[0]) and g.sync()
    covered_before = set(m.tiles_) & set(coords)
    assert covered_before                                                # keyframe 0 left bounds on tiles the import overwrites
    for t, lw in tiles.items():
        m.tiles_[t] = ([a.copy() for a in lw[0]], [a.copy() for a in lw[1]])
    m._out = {}
    pi.import_tiles(g, tiles)
    assert feed_with_model(o, m, frames[1], poses[1]) and g.feed(frames[1], poses[1]) and g.sync()
    assert g.tiles() == m.tiles()
    won = 0
    for t in m.tiles():
        for i in range(m.num_levels):
            gl, gw = g.tile_level(*t, i)
            ml, mw = m.tile_level(*t, i)
            assert np.array_equal(gw, mw), ("weight", t, i, int((gw != mw).sum()))
            assert np.array_equal(gl, ml), ("lap", t, i, int((gl != ml).sum()))
        if t in tiles:
            won += int((m.tiles_[t][1][0] != tiles[t][1][0]).sum())
    assert won > 0                                                       # the keyframe took pixels of imported tiles ...
    assert all(np.array_equal(m.tiles_[coords[1]][1][i], tiles[coords[1]][1][i]) for i in range(bands + 1))   # ... none of the 1e30 tile
    g.close()
