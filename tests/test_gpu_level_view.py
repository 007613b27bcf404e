"""The reduced-resolution views on the GPU (csrc/collapse_level.hip behind pf_blend_tiles_level, pf_blend_changed_level and
pf_save_to_memory_level) against their model (level_view_model.py), bit for bit, at every level of 1-, 5- and 8-band maps (tiles of
128 x 128 down to 1 x 1 pixels), with and without neighbours; level 0 through the new calls against the existing ones; the draw()
loop at a level; readers between feeds; refusals; page-locked against pageable outputs.  The rig is test_gpu_model.py's."""
import ctypes

import numpy as np
import pytest

from helpers import workloads
from level_view_model import lattice_model, model_blend_level, model_save_level
from map_model import to_8u
from test_gpu_model import BG, CAM

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ABSENT = (10 ** 5, -(10 ** 5))                  # a coordinate no map here holds a tile at
CAP = 32                                        # tiles a blend_changed buffer here is sized for: more than any map of the rig holds


def gpu_map(pf, force_float, bands, keep=(0, 1, 2, 3), thread=False, **opt):
    """A map fed the keyframes `keep` of the rig, and their model"""
    poses, prep, frames, m = lattice_model(force_float, bands, keep, opt.get("high_quality_show", 1))
    g = pf.Map2D.create(pf.TypeMultiBandCPU, thread, force_float=force_float, band_number=bands, bg_color=BG, **opt)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    for f, p in zip(frames, poses):
        assert g.feed(f, p)
    return g, m


def shuffled(tiles, seed):
    """the tiles in a shuffled order with a coordinate that holds no tile in the middle"""
    order = list(tiles)
    np.random.RandomState(seed).shuffle(order)
    order.insert(len(order) // 2, ABSENT)
    return order


def check_tile_views(g, m, k, seed=0):
    """all tiles in one call per output kind, raw and 8U, against the model; the absent coordinate keeps its bytes"""
    e = 256 >> k
    order = shuffled(m.tiles(), seed + k)
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
        want = model_blend_level(m, *t, k)
        assert np.array_equal(raw[i], want), (k, t, "raw", int((raw[i] != want).sum()))
        assert np.array_equal(bgr[i], to_8u(want)), (k, t, "8U", int((bgr[i] != to_8u(want)).sum()))


@pytest.mark.parametrize("high_quality_show", [1, 0])
@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
def test_tile_views_of_every_level_equal_the_model(pf, force_float, bands, high_quality_show):
    g, m = gpu_map(pf, force_float, bands, high_quality_show=high_quality_show)
    assert g.num_levels == m.num_levels == bands + 1
    if high_quality_show:                                           # a middle tile with all nine neighbours, rim tiles that blend by self
        have = set(m.tiles())
        full = [t for t in have if all((t[0] + dx, t[1] + dy) in have for dx in (-1, 0, 1) for dy in (-1, 0, 1))]
        assert full and len(full) < len(have)
    for k in range(g.num_levels):
        check_tile_views(g, m, k, seed=bands)
    g.close()


@pytest.mark.parametrize("keep", [(0, 1, 2, 3), (0, 1, 2)])
@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
def test_mosaic_views_of_every_level_equal_the_model(pf, force_float, bands, keep):
    """keep = (0, 1, 2): an L-shaped map whose bounding box holds slots without a tile -- the background colour there, and zero levels
    feeding their neighbours' pyrUp"""
    g, m = gpu_map(pf, force_float, bands, keep)
    tiles = m.tiles()
    xs, ys = [t[0] for t in tiles], [t[1] for t in tiles]
    assert len(tiles) < (max(xs) + 1 - min(xs)) * (max(ys) + 1 - min(ys))
    for k in range(g.num_levels):
        got, origin = g.save_to_memory(level=k)
        want, want_origin = model_save_level(m, k)
        assert origin == want_origin and got.shape == want.shape, k
        assert np.array_equal(got, want), (k, int((got != want).any(axis=2).sum()))
        if k == 0:
            assert (got == BG).all(axis=2).any()
    g.close()


@pytest.mark.parametrize("force_float", [0, 1])
def test_level_0_through_the_new_calls_is_the_existing_calls(pf, force_float):
    g, m = gpu_map(pf, force_float, 5)
    twin, _ = gpu_map(pf, force_float, 5)
    tiles = m.tiles()
    assert np.array_equal(g.blend_tiles(tiles, level=0), np.stack([g.blend_tile(*t) for t in tiles]))
    assert np.array_equal(g.blend_tiles_raw(tiles, level=0), np.stack([g.blend_tile_raw(*t) for t in tiles]))
    L = pf.lib()
    xy = (ctypes.c_int * (2 * len(tiles)))(*[v for t in tiles for v in t])
    old = np.zeros((len(tiles), 256, 256, 3), np.uint8)
    assert L.pf_blend_tiles(g._h, xy, len(tiles), old.ctypes.data)
    assert np.array_equal(g.blend_tiles(tiles, level=0), old)
    r, c, x0, y0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.pf_save_to_memory(g._h, None, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0))
    mosaic = np.zeros((r.value, c.value, 3), np.uint8)
    assert L.pf_save_to_memory(g._h, mosaic.ctypes.data, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0))
    new, origin = g.save_to_memory(level=0)
    assert origin == (x0.value, y0.value) and np.array_equal(new, mosaic)
    # the draw() loop: pf_blend_changed on the twin, pf_blend_changed_level(0) here -- the same list, flags cleared once
    cap = len(tiles) + 2
    xy_old = (ctypes.c_int * (2 * cap))(); px_old = np.zeros((cap, 256, 256, 3), np.uint8)
    n_old = L.pf_blend_changed(twin._h, xy_old, px_old.ctypes.data, cap)
    got_tiles, got_px = g.blend_changed(cap=cap, level=0)
    assert n_old == len(tiles) and got_tiles == [(xy_old[2 * i], xy_old[2 * i + 1]) for i in range(n_old)]
    assert np.array_equal(got_px, px_old[:n_old])
    assert g.blend_changed(cap=cap, level=0)[0] == [] and g.blend_changed(cap=cap)[0] == []
    g.close(); twin.close()


def test_blend_changed_at_a_level_is_the_draw_loop(pf):
    """two keyframes, a refresh, two more: blend_changed(level=2) returns exactly the tiles blend_changed() returns on a twin fed the
    same way, as views of level 2, and clears their flags"""
    poses, prep, frames, m = lattice_model(0, 5)
    maps = []
    for _ in range(2):
        g = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG)
        assert g.prepare(workloads().IDENTITY_PLANE, CAM, prep)
        for f, p in zip(frames[:2], poses[:2]):
            assert g.feed(f, p)
        maps.append(g)
    g, twin = maps
    first = twin.blend_changed(cap=CAP)[0]
    assert g.blend_changed(cap=CAP, level=2)[0] == first and first
    for x in maps:
        for f, p in zip(frames[2:], poses[2:]):
            assert x.feed(f, p)
    want_tiles = twin.blend_changed(cap=CAP)[0]
    got_tiles, got = g.blend_changed(cap=CAP, level=2)
    assert got_tiles == want_tiles and 0 < len(want_tiles) <= len(m.tiles()) and got.shape[1:] == (64, 64, 3)
    for t, im in zip(got_tiles, got):
        assert np.array_equal(im, to_8u(model_blend_level(m, *t, 2))), t
    assert g.blend_changed(cap=CAP, level=2)[0] == [] and g.blend_changed(cap=CAP)[0] == []
    g.close(); twin.close()


def test_a_reader_between_feeds_sees_the_keyframes_fed_so_far(pf):
    """lookahead at its default: keyframes wait to be rendered, and every level view renders them first"""
    poses, prep, frames, m4 = lattice_model(1, 5)
    _, _, _, m2 = lattice_model(1, 5, keep=(0, 1))
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=1, band_number=5, bg_color=BG)
    assert g.opt.lookahead > 0
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    for upto, m in ((2, m2), (4, m4)):
        for f, p in zip(frames[upto - 2:upto], poses[upto - 2:upto]):
            assert g.feed(f, p)
        tiles = m.tiles()
        for t, im in zip(tiles, g.blend_tiles(tiles, level=1)):
            assert np.array_equal(im, to_8u(model_blend_level(m, *t, 1))), (upto, t)
        got, origin = g.save_to_memory(level=3)
        want, want_origin = model_save_level(m, 3)
        assert origin == want_origin and np.array_equal(got, want), upto
    g.close()


def test_threaded_map_views_hold_the_rendered_keyframes(pf):
    g, _ = gpu_map(pf, 0, 5, thread=True)
    assert g.sync()
    log = g.render_log()
    assert log and log == sorted(log)
    _, _, _, m = lattice_model(0, 5, keep=tuple(log))              # the model holds what the worker rendered
    check_tile_views(g, m, 2)
    got, origin = g.save_to_memory(level=2)
    want, want_origin = model_save_level(m, 2)
    assert origin == want_origin and np.array_equal(got, want)
    g.close()


def refused(pf, g, tiles, level):
    """every call at `level` returns nothing, names a reason and leaves the outputs and the Ischanged flags alone"""
    L = pf.lib()
    n = len(tiles)
    out = np.full((n + 1, 256, 256, 3), SENTINEL, np.uint8)
    raw = np.full((n + 1, 256, 256, 3 * 4), SENTINEL, np.uint8)
    xy = (ctypes.c_int * (2 * (n + 1)))(*([v for t in tiles for v in t] + [SENTINEL, SENTINEL]))
    r, c, x0, y0 = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    for call in (lambda: L.pf_blend_tiles_level(g._h, xy, n, level, out.ctypes.data, raw.ctypes.data),
                 lambda: L.pf_blend_changed_level(g._h, level, xy, out.ctypes.data, n + 1),
                 lambda: L.pf_save_to_memory_level(g._h, level, None, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0)),
                 lambda: L.pf_save_to_memory_level(g._h, level, out.ctypes.data, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0))):
        assert call() == 0
        msg = L.pf_last_error().decode()
        assert msg and "level" in msg, msg
    assert (out == SENTINEL).all() and (raw == SENTINEL).all() and (r.value, c.value, x0.value, y0.value) == (7, 7, 7, 7)
    assert list(xy)[-2:] == [SENTINEL, SENTINEL] and list(xy)[:2 * n] == [v for t in tiles for v in t]
    assert g.blend_tiles(tiles, level=level) is None and g.save_to_memory(level=level) is None


def test_refusals_touch_nothing_and_name_the_reason(pf):
    wl = workloads()
    poses, prep, frames, m = lattice_model(0, 5)
    tiles = m.tiles()
    g, _ = gpu_map(pf, 0, 5)
    for level in (-1, g.num_levels):
        refused(pf, g, tiles, level)
    check_tile_views(g, m, g.num_levels - 1)                       # the top level is the last one there is
    assert len(g.blend_changed(cap=CAP, level=0)[0]) == len(tiles)  # the refused draw loops cleared no flag
    g.close()

    single = pf.Map2D.create(pf.TypeCPU, False)
    sharded = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG, shard_rank=0, shard_count=2, shard_block=1)
    for x in (single, sharded):
        assert x.prepare(wl.IDENTITY_PLANE, CAM, prep)
        for f, p in zip(frames, poses):
            assert x.feed(f, p)
        held = x.tiles()
        assert held and (x is single or len(held) < len(tiles))     # the shard holds a part of the map
        refused(pf, x, held, 1)
        # level 0 still works there, through the new calls as through the old
        assert np.array_equal(x.blend_tiles(held, level=0), np.stack([x.blend_tile(*t) for t in held]))
        new, origin = x.save_to_memory(level=0)
        old = np.zeros_like(new)
        r, c, x0, y0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert pf.lib().pf_save_to_memory(x._h, old.ctypes.data, ctypes.byref(r), ctypes.byref(c), ctypes.byref(x0), ctypes.byref(y0))
        assert np.array_equal(new, old) and origin == (x0.value, y0.value)
        changed, px = x.blend_changed(cap=CAP, level=0)
        assert sorted(changed) == sorted(held) and px.shape[1:] == (256, 256, 3)
        x.close()


@pytest.mark.parametrize("force_float", [0, 1])
def test_page_locked_outputs_equal_pageable_ones(pf, force_float):
    g, m = gpu_map(pf, force_float, 5)
    tiles = m.tiles()
    for k in (1, 3):
        e = 256 >> k
        pinned = pf.host_array((len(tiles), e, e, 3)); pinned[:] = SENTINEL
        assert g.blend_tiles(tiles, out=pinned, level=k) is not None
        assert np.array_equal(pinned, g.blend_tiles(tiles, level=k))
        pinned_raw = pf.host_array((len(tiles), e, e, 3), g.dtype)
        assert g.blend_tiles_raw(tiles, level=k, out=pinned_raw) is not None
        assert np.array_equal(pinned_raw, g.blend_tiles_raw(tiles, level=k))
        a, origin_a = g.save_to_memory(alloc=pf.host_array, level=k)
        b, origin_b = g.save_to_memory(level=k)
        assert origin_a == origin_b and np.array_equal(a, b) and np.array_equal(b, model_save_level(m, k)[0])
    g.close()
