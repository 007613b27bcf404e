"""The rule of the map merge, pinned on the CPU against the oracle alone (no HIP code runs here): because canvases are tile aligned, a
keyframe that touches a tile covers all of it at every level, so the map fed sortie A and then sortie B is -- tile by tile, level by
level, bit for bit -- the map fed A merged with the map fed B by the render's own select with B's tile as the newer keyframe:
    multi-band   if (srcW >= dstW) { dstL = srcL; dstW = srcW; }      (MultiBandMap2DCPU.cpp:521,542)
    single band  if (dst.a < src.a) dst = src                          (Map2DCPU.cpp:326: ties keep dst)
a tile only src holds is copied, a tile only dst holds is left alone.  The workload (merge_workload.py) shares one pose between the
sorties, so whole tiles tie, and the reversed order gives another map: the rule's tie direction and order are both visible."""
import numpy as np
import pytest

from merge_workload import oracle_fed


def merged_levels(a, b, t, lv):
    """tile t, level lv of `a merged with b` under the rule; None where neither holds the tile"""
    ta, tb = a.tile_level(t[0], t[1], lv) if t in a.tiles() else None, b.tile_level(t[0], t[1], lv) if t in b.tiles() else None
    if ta is None or tb is None:
        return ta if tb is None else tb
    win = tb[1] >= ta[1]
    return np.where(win[:, :, None], tb[0], ta[0]), np.where(win, tb[1], ta[1])


def mismatching_tile_levels(a, b, ref):
    bad = 0
    for t in ref.tiles():
        for lv in range(ref.num_levels):
            m, r = merged_levels(a, b, t, lv), ref.tile_level(t[0], t[1], lv)
            bad += not (m is not None and np.array_equal(m[0], r[0]) and np.array_equal(m[1], r[1]))
    return bad


@pytest.mark.parametrize("ff", [0, 1])
@pytest.mark.parametrize("bands", [2, 5, 7])
def test_merge_rule_equals_sequential_feed(orc, ff, bands):
    a, b = oracle_fed("A", "AB", ff, bands), oracle_fed("B", "AB", ff, bands)
    ab, ba = oracle_fed("AB", "AB", ff, bands), oracle_fed("BA", "AB", ff, bands)
    both = set(a.tiles()) & set(b.tiles())
    assert sorted(set(a.tiles()) | set(b.tiles()), key=lambda t: t[::-1]) == ab.tiles() == ba.tiles()
    assert len(ab.tiles()) == 19 and len(both) == 15
    assert mismatching_tile_levels(a, b, ab) == 0
    assert mismatching_tile_levels(b, a, ba) == 0
    # the order matters, and the rule follows it: A merged with B is not the map fed B and then A
    assert mismatching_tile_levels(a, b, ba) > 0 and mismatching_tile_levels(b, a, ab) > 0


def merged_bgra(a, b, t):
    ta, tb = a.tile_bgra(*t) if t in a.tiles() else None, b.tile_bgra(*t) if t in b.tiles() else None
    if ta is None or tb is None:
        return ta if tb is None else tb
    return np.where((ta[:, :, 3] < tb[:, :, 3])[:, :, None], tb, ta)


def test_single_band_rule_equals_sequential_feed(orc):
    a, b = oracle_fed("A", "AB", single_band=1), oracle_fed("B", "AB", single_band=1)
    ab, ba = oracle_fed("AB", "AB", single_band=1), oracle_fed("BA", "AB", single_band=1)
    assert sorted(set(a.tiles()) | set(b.tiles()), key=lambda t: t[::-1]) == ab.tiles() == ba.tiles() and len(ab.tiles()) == 19
    assert all(np.array_equal(merged_bgra(a, b, t), ab.tile_bgra(*t)) for t in ab.tiles())
    assert all(np.array_equal(merged_bgra(b, a, t), ba.tile_bgra(*t)) for t in ba.tiles())
    assert sum(not np.array_equal(merged_bgra(a, b, t), ba.tile_bgra(*t)) for t in ba.tiles()) > 0


def test_far_sortie_leaves_the_prepared_grid_and_shares_no_tile(orc):
    """the growth case of test_gpu_merge.py: F's tiles are all new to a map fed A, and the grid prepared from A alone has to grow for them"""
    a, f, af = oracle_fed("A", "A"), oracle_fed("F", "A"), oracle_fed("AF", "A")
    assert not set(a.tiles()) & set(f.tiles()) and sorted(set(a.tiles()) | set(f.tiles()), key=lambda t: t[::-1]) == af.tiles()
    assert a.grid()[0] != af.grid()[0] and f.grid()[0] == af.grid()[0]
