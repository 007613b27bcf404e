"""The merge kernels (csrc/merge.hip: k_merge<F32>, k_merge_bgra) and their driver (FusionMap::merge_items, merge_records) on slot
images that no keyframe leaves behind (merge_slots.py), product library.  dst images go into an empty prepared map through
tile_import (padding 0x3C), src images lie in one tensor with guard bytes around each (padding 0xA5) and are merged through
merge_tiles, or through a state file written by hand; afterwards every tile is exported whole and compared with the byte-level model
(tests/test_merge_slots.py ties that model to the oracle), padding included.  Pinned here and nowhere else: the scalar tail at
every band count, the first and last item of every level, groups won lane by lane, `>=` on ties, -0.0, NaN, +-inf, denormals and
negative weights, `<` on the alpha byte alone, the bytes of a slot that belong to no level, the second launch of a merge of more
than 512 pairs, the second staging batch of a state file, and the `won` counter.  Every comparison is on bytes and exact."""
import numpy as np
import pytest

import merge_slots as ms
import pyramid_inject as pi
import state_files as sf

pytestmark = pytest.mark.gpu


def err(pf):
    return pf.lib().pf_last_error().decode()


def by_row(tiles):
    return sorted(tiles, key=lambda t: t[::-1])


def to_device(a):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                                             # the map works on a stream of its own: the upload comes first
    return dev


def import_held(g, cases):
    for c in cases:
        if c["dst"] is not None:
            dev = to_device(c["dst"])
            assert g.tile_import(c["t"][0], c["t"][1], dev.data_ptr()), c["t"]


def upload_sources(images):
    """the src images in one uint8 tensor, ms.GUARD bytes of 0x5A before and behind each; returns (tensor, its host copy, addresses)"""
    total = images[0].size
    stride = total + 2 * ms.GUARD
    host = np.full((len(images), stride), ms.GUARD_BYTE, np.uint8)
    for k, im in enumerate(images):
        host[k, ms.GUARD:ms.GUARD + total] = im
    dev = to_device(host)
    assert dev.data_ptr() % 16 == 0 and stride % 16 == 0
    return dev, host, [dev.data_ptr() + k * stride + ms.GUARD for k in range(len(images))]


def export_all(g, tiles):
    """{t: the tile's slot image, exported whole}; the guard bytes behind every image must come back untouched"""
    import torch
    total = g.tile_bytes()
    buf = torch.full((len(tiles), total + ms.GUARD), ms.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k, t in enumerate(tiles):
        assert g.tile_export(t[0], t[1], buf[k].data_ptr()), t
    got = buf.cpu().numpy()
    assert (got[:, total:] == ms.GUARD_BYTE).all()
    return {t: got[k, :total] for k, t in enumerate(tiles)}


def assert_tiles(g, want):
    """the map holds exactly want's tiles, and each is want's bytes"""
    assert g.tiles() == by_row(want)
    got = export_all(g, g.tiles())
    for t, w in want.items():
        if not np.array_equal(got[t], w):
            at = np.flatnonzero(got[t] != w)
            raise AssertionError("tile %s: %d bytes differ, first at %d: got 0x%02x, want 0x%02x" % (t, at.size, at[0], got[t][at[0]], w[at[0]]))


def merge_and_check(pf, g, cases, images=None, bands=0, ff=0, single=False, order=None):
    """dst's tiles imported, the src images merged in one merge_tiles, everything compared with the model"""
    assert g.tile_bytes() == (256 * 256 * 4 if single else pi.slot_layout(bands, ff)["total"])
    import_held(g, cases)
    assert g.tiles() == by_row(c["t"] for c in cases if c["dst"] is not None)
    pairs = [c for c in cases if c["src"] is not None]
    if order is not None:
        pairs = [pairs[k] for k in order]
    dev, host, ptrs = upload_sources(images if images is not None else [c["src"] for c in pairs])
    g.merge_stats(count_stores=True)
    assert g.merge_tiles([c["t"] for c in pairs], [ptrs[c["src"] if images is not None else k] for k, c in enumerate(pairs)], None), err(pf)
    st = g.merge_stats()
    want, won, n_pairs, n_fresh = ms.expected(cases, images, bands, ff, single)
    assert (st["pairs"], st["fresh"], st["slot_bytes"]) == (n_pairs, n_fresh, g.tile_bytes())
    assert st["won"] == won
    assert_tiles(g, want)
    assert np.array_equal(dev.cpu().numpy(), host)                       # src and its guards: bit-identical to what was uploaded
    return want


# ---------------------------------------------------------------- every band count and type
@pytest.mark.parametrize("ff", [0, 1])
@pytest.mark.parametrize("bands", ms.BANDS)
def test_every_kind_at_every_band_count(pf, bands, ff):
    """one merge per band count and type (merge_slots.merge_cases): three phases of mixed, lone winners and losers, ties, specials as
    tiles dst holds, two fresh tiles, one tile only dst holds; the pairs are given in the reverse of the store's order"""
    cases = ms.merge_cases(bands, ff)
    g = pi.new_map(pf, bands, ff)
    n = sum(c["src"] is not None for c in cases)
    want = merge_and_check(pf, g, cases, bands=bands, ff=ff, order=list(range(n))[::-1])
    lone = next(c for c in cases if c["kind"] == "dst_only")
    assert want[lone["t"]].tobytes() == lone["dst"].tobytes()
    g.close()


def test_single_band_kinds(pf):
    """k_merge_bgra: the same kinds on the alpha byte, an equal-alpha tie in both directions (dst keeps its colours each time)"""
    cases = ms.bgra_cases()
    g = ms.new_single_band_map(pf)
    n = sum(c["src"] is not None for c in cases)
    want = merge_and_check(pf, g, cases, single=True, order=list(range(n))[::-1])
    for c in cases:
        if c["kind"] in ("ties", "ties_swapped", "dst_only"):
            assert want[c["t"]].tobytes() == c["dst"].tobytes()
    g.close()


# ---------------------------------------------------------------- more pairs than one launch takes
def test_merge_of_515_pairs_across_the_launch_batch(pf):
    """0 bands, 16S: 515 pairs in one merge_tiles, two launches from one table; dst holds the pairs at both ends of the first launch
    and around the start of the second, four src images serve all pairs"""
    cases, images = ms.batch_cases()
    g = pi.new_map(pf, 0, 0)
    merge_and_check(pf, g, cases, images, bands=0, ff=0)
    g.close()


# ---------------------------------------------------------------- a state file of more than one staging batch
def wide_map(pf, bands, ff):
    from helpers import workloads
    from test_gpu_model import CAM
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, band_number=bands, bg_color=pi.BG)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, ms.wide_poses(bands))
    return g


def test_state_file_in_two_staging_batches(pf, tmp_path):
    """8 bands, 32F: a file of 26 records written by hand under a real empty map's header; 23 records fill the staging memory, the
    other three reuse it.  load_state gives the file's images back, padding as written; merge_state into a map that holds `mixed`
    tiles at the last two records of batch one and the first two of batch two equals the model; save_state of the loaded map is
    the file with its gaps zeroed."""
    bands, ff = 8, 1
    p0, p1, p2 = (str(tmp_path / n) for n in ("empty.pfstate", "hand.pfstate", "saved.pfstate"))
    dst = wide_map(pf, bands, ff)
    assert dst.save_state(p0), err(pf)
    head = open(p0, "rb").read()
    assert len(head) == sf.HEADER_BYTES
    w, h, ox, oy = sf.grid_of(head)
    total = dst.tile_bytes()
    n = ms.STAGE_BYTES // total + 3
    coords = [(ox + x, oy + y) for y in range(h) for x in range(w)][:n]
    assert len(coords) == n == 26
    cases, first = ms.state_cases(coords, bands, ff)
    body = b"".join(sf.record(c["t"][0], c["t"][1], total, image=c["src"]) for c in cases)
    with open(p1, "wb") as f:
        f.write(sf.with_tile_count(head, n) + body)
    assert pf.state_info(p1)["tiles"] == n, err(pf)

    loaded = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, band_number=bands, bg_color=pi.BG)
    assert loaded.load_state(p1), err(pf)
    assert_tiles(loaded, {c["t"]: c["src"] for c in cases})
    assert loaded.grid() == dst.grid()
    assert loaded.save_state(p2), err(pf)
    zeroed = b"".join(sf.record(c["t"][0], c["t"][1], total, image=ms.zero_gaps(c["src"], bands, ff)) for c in cases)
    assert open(p2, "rb").read() == sf.with_tile_count(head, n) + zeroed

    import_held(dst, cases)
    dst.merge_stats(count_stores=True)
    assert dst.merge_state(p1), err(pf)
    want, _, _, _ = ms.expected(cases, None, bands, ff)
    assert_tiles(dst, want)
    # the statistics are the last merge's: batch two, three records, two of them over tiles dst held
    _, won, pairs, fresh = ms.expected(cases[first:], None, bands, ff)
    st = dst.merge_stats()
    assert (st["pairs"], st["fresh"], st["won"]) == (pairs, fresh, won) == (3, 1, won)
    dst.close(); loaded.close()


# ---------------------------------------------------------------- refusals
def test_refused_merge_tiles_leaves_every_byte(pf):
    """the duplicate-coordinate and the misaligned-pointer refusals of merge_tiles: dst's hostile tiles, src's images and the tile
    list are what they were, bit for bit"""
    bands, ff = 5, 1
    cases = [c for c in ms.merge_cases(bands, ff) if c["kind"] in ("mixed", "specials", "ties")]
    g = pi.new_map(pf, bands, ff)
    import_held(g, cases)
    before = {c["t"]: c["dst"] for c in cases}
    dev, host, ptrs = upload_sources([c["src"] for c in cases])
    tiles = [c["t"] for c in cases]
    g.merge_stats(count_stores=True)
    assert not g.merge_tiles(tiles + tiles[:1], ptrs + ptrs[:1], None) and "twice" in err(pf)
    assert_tiles(g, before)
    assert not g.merge_tiles(tiles, ptrs[:-1] + [ptrs[-1] + 4], None) and "aligned" in err(pf)
    assert_tiles(g, before)
    assert np.array_equal(dev.cpu().numpy(), host)
    # and the same call without the flaw merges
    assert g.merge_tiles(tiles, ptrs, None), err(pf)
    assert_tiles(g, ms.expected(cases, None, bands, ff)[0])
    g.close()
