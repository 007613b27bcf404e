"""Map merge and the state file on the GPU (csrc/merge.hip, FusionMap::merge_from / merge_tiles / save_state / load_state / merge_state),
product library, default lookahead.  The reference is the oracle fed the same keyframes in sequence: a merged map must equal it bit for
bit, tile by tile and level by level (tests/test_merge_model.py pins that rule on the CPU).  Workload: merge_workload.py, 640 x 480,
19 tiles, one pose shared between the two sorties so that whole tiles tie in weight."""
import os

import numpy as np
import pytest

import state_files as sf
from helpers import compare_maps, map_digest, workloads
from merge_workload import CAM, feed, oracle_fed, poses_of

pytestmark = pytest.mark.gpu


def err(pf):
    return pf.lib().pf_last_error().decode()


def fed(pf, names, prep="AB", thread=False, type=None, sync=True, **opt):
    """a HIP map prepared with the poses of sorties `prep` and fed the sorties `names`"""
    g = pf.Map2D.create(pf.TypeMultiBandCPU if type is None else type, thread, **opt)
    if prep:
        assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses_of(prep))
    feed(g, names)
    if sync:
        assert g.sync()
    return g


def bounds(g):
    return {t: g.tile_bounds(*t).tolist() for t in g.tiles()}


def export_all(g):
    """(tiles, torch uint8 tensor n x tile_bytes on the GPU, n x 16 bounds) of map g"""
    import torch
    tiles = g.tiles()
    buf = torch.empty((len(tiles), g.tile_bytes()), dtype=torch.uint8, device="cuda")
    for k, t in enumerate(tiles):
        assert g.tile_export(t[0], t[1], buf[k].data_ptr())
    return tiles, buf, np.stack([g.tile_bounds(*t) for t in tiles])


# ------------------------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("ff", [0, 1])
@pytest.mark.parametrize("bands", [2, 5, 7])
def test_merge_equals_sequential_feed(pf, orc, ff, bands):
    opt = dict(force_float=ff, band_number=bands)
    g1, g2 = fed(pf, "A", **opt), fed(pf, "B", **opt)
    before = map_digest(g2)
    assert g1.merge(g2), err(pf)
    assert compare_maps(g1, oracle_fed("AB", "AB", ff, bands)) == []
    assert map_digest(g2) == before and compare_maps(g2, oracle_fed("B", "AB", ff, bands)) == []
    st = g1.merge_stats()
    # every tile src holds is a pair; those dst did not hold are copies
    assert st["pairs"] == len(g2.tiles()) and st["fresh"] == len(set(g2.tiles()) - set(oracle_fed("A", "AB", ff, bands).tiles()))
    # the other way round: the map fed B and then A
    r1, r2 = fed(pf, "B", **opt), fed(pf, "A", **opt)
    assert r1.merge(r2), err(pf)
    assert compare_maps(r1, oracle_fed("BA", "AB", ff, bands)) == []
    for g in (g1, g2, r1, r2):
        g.close()


@pytest.mark.parametrize("thread", [False, True])
def test_merge_with_keyframes_still_waiting(pf, orc, thread):
    """no sync() before the merge: keyframes wait in both lookahead windows, or in the feed queues of thread = 1 maps"""
    g1, g2 = fed(pf, "A", thread=thread, sync=False), fed(pf, "B", thread=thread, sync=False)
    assert g1.merge(g2), err(pf)
    assert compare_maps(g1, oracle_fed("AB", "AB")) == []
    assert compare_maps(g2, oracle_fed("B", "AB")) == []
    g1.close(); g2.close()


def test_single_band_merge(pf, orc):
    for order in ("AB", "BA"):
        g1, g2 = fed(pf, order[0], type=pf.TypeCPU), fed(pf, order[1], type=pf.TypeCPU)
        src_before = {t: g2.tile_bgra(*t) for t in g2.tiles()}
        assert g1.merge(g2), err(pf)
        o = oracle_fed(order, "AB", single_band=1)
        assert g1.tiles() == o.tiles() and len(o.tiles()) == 19
        bad = [t for t in o.tiles() if not np.array_equal(g1.tile_bgra(*t), o.tile_bgra(*t))]
        assert bad == [], (order, bad)
        assert all(np.array_equal(g2.tile_bgra(*t), v) for t, v in src_before.items())
        g1.close(); g2.close()


def test_only_src_holds_tiles_and_the_grid_grows(pf, orc):
    """both maps prepared from A alone; F is flown far outside that grid and shares no tile with A: every pair is a copy into a new tile,
    and dst's grid has to grow to src's.  Tiles, dims and output equal the oracle fed A then F; geo to 1e-12 (min_ is reached by another
    chain of min + ele_size * k than in the sequential map and may differ in the last bit)."""
    g1, g2 = fed(pf, "A", prep="A"), fed(pf, "F", prep="A")
    o = oracle_fed("AF", "A")
    assert g1.grid()[0] != o.grid()[0]
    assert g1.merge(g2), err(pf)
    assert g1.merge_stats()["fresh"] == g1.merge_stats()["pairs"] == len(g2.tiles()) > 0
    assert compare_maps(g1, o) == []
    (dims, geo), (odims, ogeo) = g1.grid(), o.grid()
    assert dims == odims
    assert np.allclose(geo, ogeo, rtol=1e-12, atol=0)
    (img, org), (oimg, oorg) = g1.save_to_memory(), o.save()
    assert tuple(org) == tuple(oorg) and img.shape == oimg.shape and np.array_equal(img, oimg)
    g1.close(); g2.close()


def check_against_oracle_abc(g, o):
    assert compare_maps(g, o) == []
    bad = [t for t in o.tiles() if not np.array_equal(g.blend_tile(*t), o.blend_tile(*t))]
    assert bad == []
    (img, org), (oimg, oorg) = g.save_to_memory(), o.save()
    assert tuple(org) == tuple(oorg) and img.shape == oimg.shape and np.array_equal(img, oimg)


def test_life_goes_on_after_a_merge(pf, orc):
    """prepared with every sortie's poses (no growth: the case for which feeding after a merge is guaranteed to equal the oracle), merged,
    then four more keyframes with the cull on: they are culled against both maps' bounds, and the map is the oracle's fed A, B, C"""
    o = oracle_fed("ABC", "ABC")
    g1, g2 = fed(pf, "A", prep="ABC"), fed(pf, "B", prep="ABC")
    assert g1.merge(g2), err(pf)
    culled = g1.culled_cells() + g1.culled_tiles()
    feed(g1, "C")
    assert g1.sync()
    check_against_oracle_abc(g1, o)
    assert g1.culled_cells() + g1.culled_tiles() > culled
    # the same through tile_export -> merge_tiles without bounds: nothing is known of the foreign tiles' weights, the map is the same
    h1 = fed(pf, "A", prep="ABC")
    tiles, buf, _ = export_all(g2)
    assert h1.merge_tiles(tiles, [buf[k].data_ptr() for k in range(len(tiles))], None), err(pf)
    feed(h1, "C")
    assert h1.sync()
    assert map_digest(h1) == map_digest(g1)
    check_against_oracle_abc(h1, o)
    for g in (g1, g2, h1):
        g.close()


def test_merge_tiles_with_bounds_equals_merge(pf, orc):
    g1, g2, h1 = fed(pf, "A"), fed(pf, "B"), fed(pf, "A")
    assert g1.merge(g2), err(pf)
    tiles, buf, wlb = export_all(g2)
    ptrs = [buf[k].data_ptr() for k in range(len(tiles))]
    before, grid = map_digest(h1), h1.grid()
    assert not h1.merge_tiles(tiles + tiles[:1], ptrs + ptrs[:1], None) and "twice" in err(pf)
    assert not h1.merge_tiles(tiles, [ptrs[0] + 4] + ptrs[1:], None) and "aligned" in err(pf)
    assert map_digest(h1) == before and h1.grid() == grid
    assert h1.merge_tiles(tiles, ptrs, wlb), err(pf)
    assert map_digest(h1) == map_digest(g1) and compare_maps(h1, oracle_fed("AB", "AB")) == []
    assert bounds(h1) == bounds(g1)
    # the max rule: no bound of the merged map is below dst's own or src's
    h2 = fed(pf, "A")
    a, b, m = bounds(h2), bounds(g2), bounds(g1)
    for t, v in m.items():
        assert v == np.maximum(a.get(t, [-1.0] * 16), b.get(t, [-1.0] * 16)).tolist(), t
    # a bound that is not finite counts as unknown: the tile keeps dst's own bound there, a new tile has none
    nan = wlb.copy(); nan[:, 0] = np.nan; nan[:, 1] = np.inf
    assert h2.merge_tiles(tiles, ptrs, nan), err(pf)
    assert map_digest(h2) == map_digest(g1)
    for t, v in bounds(h2).items():
        assert v[:2] == a.get(t, [-1.0] * 16)[:2] and v[2:] == m[t][2:], t
    for g in (g1, g2, h1, h2):
        g.close()


def test_refusals_touch_nothing(pf, orc):
    dst = fed(pf, "A")
    before, grid = map_digest(dst), dst.grid()
    others = {
        "unprepared": fed(pf, "", prep=None),
        "band_number": fed(pf, "B", band_number=4),
        "force_float": fed(pf, "B", force_float=1),
        "map type": fed(pf, "B", type=pf.TypeCPU),
        "weight_type": fed(pf, "B", weight_type=1),
        "prepare": fed(pf, "B", prep="B"),
        "sharded": fed(pf, "B", shard_count=2, shard_rank=0),
    }
    assert not dst.merge(dst) and err(pf).startswith("merge: ")
    for what, src in others.items():
        sd = map_digest(src) if what not in ("unprepared", "map type") else None
        assert not dst.merge(src), what
        assert err(pf).startswith("merge: "), (what, err(pf))
        assert not src.merge(dst), what                           # and the other way round
        assert err(pf).startswith("merge: "), (what, err(pf))
        assert map_digest(dst) == before and dst.grid() == grid, what
        if sd is not None:
            assert map_digest(src) == sd, what
    assert others["unprepared"].grid() is None
    for g in list(others.values()) + [dst]:
        g.close()


# ------------------------------------------------------------------------------------------------------------- state file
def test_state_file_round_trip_and_resume(pf, orc, tmp_path):
    p1, p2, p3 = (str(tmp_path / n) for n in ("a.pfstate", "b.pfstate", "c.pfstate"))
    g, g2 = fed(pf, "A", prep="ABC"), fed(pf, "B", prep="ABC")
    assert g.merge(g2), err(pf)
    assert g.save_state(p1) and g.save_state(p2), err(pf)
    data = open(p1, "rb").read()
    assert data == open(p2, "rb").read() and not os.path.exists(p1 + ".part")
    info = pf.state_info(p1)
    assert (info["type"], info["pyramid_type"], info["band_number"], info["weight_type"], info["tiles"]) == (pf.TypeMultiBandCPU, pf.PF_16SC3, 5, 0, len(g.tiles()))
    assert [info["w"], info["h"]] == g.grid()[0][:2] and info["geo"] == g.grid()[1] and info["cam"] == [float(v) for v in CAM]
    r = pf.Map2D.create(pf.TypeMultiBandCPU, False)
    assert r.load_state(p1), err(pf)
    assert map_digest(r) == map_digest(g) and r.grid() == g.grid() and bounds(r) == bounds(g)
    assert r.save_state(p3) and open(p3, "rb").read() == data
    # the flight goes on, in the map that never stopped and in the restored one
    c0 = [m.culled_cells() + m.culled_tiles() for m in (g, r)]
    for m in (g, r):
        feed(m, "C")
        assert m.sync()
    assert map_digest(r) == map_digest(g)
    check_against_oracle_abc(r, oracle_fed("ABC", "ABC"))
    assert compare_maps(g, oracle_fed("ABC", "ABC")) == []
    grew = [m.culled_cells() + m.culled_tiles() - c for m, c in zip((g, r), c0)]
    assert grew[1] > 0 and grew[1] == grew[0]
    # a failed save leaves no file
    nowhere = str(tmp_path / "no_such_dir" / "x.pfstate")
    assert not g.save_state(nowhere) and not os.path.exists(nowhere) and not os.path.exists(nowhere + ".part")
    for m in (g, g2, r):
        m.close()


def test_merge_state_equals_merge(pf, orc, tmp_path):
    p = str(tmp_path / "b.pfstate")
    a1, a2, b = fed(pf, "A"), fed(pf, "A"), fed(pf, "B")
    assert b.save_state(p), err(pf)
    assert a1.merge_state(p), err(pf)
    assert a2.merge(b), err(pf)
    assert map_digest(a1) == map_digest(a2) and bounds(a1) == bounds(a2) and a1.grid() == a2.grid()
    assert compare_maps(a1, oracle_fed("AB", "AB")) == []
    # a file of a map prepared otherwise, or of other options, is refused like the map itself
    other = fed(pf, "B", prep="B")
    assert other.save_state(p)
    before = map_digest(a1)
    assert not a1.merge_state(p) and err(pf).startswith("merge_state: ")
    assert map_digest(a1) == before
    for m in (a1, a2, b, other):
        m.close()


def test_hostile_files_and_other_options_leave_the_map_unchanged(pf, orc, tmp_path):
    g = fed(pf, "A", band_number=2)
    before, grid = map_digest(g), g.grid()
    p = str(tmp_path / "h.pfstate")
    hostile = sf.hostile_files(band_number=2)
    for name, data in hostile.items():
        with open(p, "wb") as f:
            f.write(data)
        assert not g.load_state(p), name
        assert err(pf).startswith("load_state: "), (name, err(pf))
        assert not g.merge_state(p), name
    assert not g.load_state(str(tmp_path / "no_such_file"))
    assert map_digest(g) == before and g.grid() == grid
    # a good file of this map, offered to maps created with other options
    assert g.save_state(p), err(pf)
    for opt in (dict(band_number=3), dict(force_float=1, band_number=2), dict(weight_type=1, band_number=2), dict(type=pf.TypeCPU)):
        m = fed(pf, "", prep=None, **opt)
        assert not m.load_state(p) and "options" in err(pf), opt
        assert m.grid() is None
        m.close()
    m = fed(pf, "", prep=None, band_number=2)
    assert m.load_state(p), err(pf)
    assert map_digest(m) == before and m.grid() == grid
    m.close(); g.close()
