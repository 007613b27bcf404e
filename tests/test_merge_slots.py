"""The byte-level merge model and its generators (merge_slots.py) without a GPU; no HIP code runs here.  The model is tied to the
reference once -- packed oracle tiles of sortie A merged with sortie B's give the oracle fed A then B, exactly -- so that
tests/test_gpu_merge_slots.py needs the model alone.  The rest are conditions on that file's inputs, for exactly the parameters it
uses (merge_cases, bgra_cases, batch_cases, state_cases): every path of csrc/merge.hip the cases are there for is reached.  A
generator that stops reaching one fails here."""
import functools

import numpy as np
import pytest

import merge_slots as ms
import pyramid_inject as pi
from merge_workload import oracle_fed


def level_wins(c, bands, ff):
    """per level the flat win mask of a case both maps hold, from the packed images the GPU test uploads"""
    (_, dw), (_, sw) = pi.unpack(c["dst"], bands, ff), pi.unpack(c["src"], bands, ff)
    return [ms.wins_of(d, s) for d, s in zip(dw, sw)]


def group_kinds(win, gpx):
    """{"all", "none", "part"} met by the groups of one vector level"""
    per = win.reshape(-1, gpx).sum(axis=1)
    return {k for k, hit in (("all", per == gpx), ("none", per == 0), ("part", (per > 0) & (per < gpx))) if hit.any()}


@functools.lru_cache(maxsize=None)
def cases_of(bands, ff):
    return ms.merge_cases(bands, ff)


# ---------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("ff,bands", [(0, 5), (1, 7)])
def test_model_on_packed_oracle_tiles_equals_sequential_feed(orc, ff, bands):
    a, b, ab = (oracle_fed(n, "AB", ff, bands) for n in ("A", "B", "AB"))
    shared = sorted(set(a.tiles()) & set(b.tiles()))
    assert len(shared) == 15
    nlev = ab.num_levels
    won = 0
    for t in shared:
        da, db = ([m.tile_level(t[0], t[1], i) for i in range(nlev)] for m in (a, b))
        dst = pi.pack([l for l, _ in da], [w for _, w in da], pad=ms.DST_PAD)
        src = pi.pack([l for l, _ in db], [w for _, w in db], pad=ms.SRC_PAD)
        got, n = ms.merge_slot(dst, src, bands, ff, False)
        won += n
        lap, w = pi.unpack(got, bands, ff)
        for i in range(nlev):
            rl, rw = ab.tile_level(t[0], t[1], i)
            assert lap[i].tobytes() == rl.tobytes() and w[i].tobytes() == rw.tobytes(), (t, i)
        assert (pi.padding_of(got, bands, ff) == ms.DST_PAD).all()
        fresh, n0 = ms.merge_slot(dst, src, bands, ff, True)
        assert fresh.tobytes() == src.tobytes() and n0 == 0
    assert 0 < won < len(shared) * sum((256 >> i) ** 2 for i in range(nlev))      # B won some pixel-levels and lost some


def test_model_moves_bits_and_keeps_every_other_byte():
    """fp32, 8 bands: a NaN weight on either side keeps dst; a winning pixel moves src's NaN payloads and -0.0 unchanged; dst's padding
    stays; a fresh slot is src's image whole"""
    bands, ff = 8, 1
    (dl, dw), (sl, sw) = ms.make_pair("specials", bands, ff, np.random.default_rng(5))
    dst, src = pi.pack(dl, dw, pad=ms.DST_PAD), pi.pack(sl, sw, pad=ms.SRC_PAD)
    got, won = ms.merge_slot(dst, src, bands, ff, False)
    lap, w = pi.unpack(got, bands, ff)
    win = ms.wins_of(dw[0], sw[0]).reshape(256, 256)
    nan = np.isnan(dw[0]) | np.isnan(sw[0])
    assert nan.any() and not win[nan].any() and win.any() and not win.all()
    assert np.array_equal(w[0].view(np.uint32), np.where(win, sw[0].view(np.uint32), dw[0].view(np.uint32)))
    assert np.array_equal(lap[0].view(np.uint32), np.where(win[:, :, None], sl[0].view(np.uint32), dl[0].view(np.uint32)))
    moved = sl[0].view(np.uint32)[win]
    assert (moved == 0xFFC12345).any() and (moved == 0x7F800001).any() and (moved == 0x80000000).any()
    # -0.0 against +0.0 is a tie: src's bits end in dst
    zz = (dw[0].view(np.uint32) == 0) & (sw[0].view(np.uint32) == 0x80000000)
    assert zz.any() and (w[0].view(np.uint32)[zz] == 0x80000000).all()
    pad = pi.padding_of(got, bands, ff)
    assert pad.size > 0 and (pad == ms.DST_PAD).all() and won == sum(int(ms.wins_of(d, s).sum()) for d, s in zip(dw, sw))
    assert ms.merge_slot(dst, src, bands, ff, True)[0].tobytes() == src.tobytes()
    assert (pi.padding_of(ms.zero_gaps(src, bands, ff), bands, ff) == 0).all()
    assert ms.padding_mask(bands, ff).sum() == pad.size


def test_bgra_model_keeps_dst_on_equal_alpha():
    dst, src = ms.make_pair_bgra("ties", np.random.default_rng(3))
    assert np.array_equal(dst[:, :, 3], src[:, :, 3]) and (dst[:, :, :3] != src[:, :, :3]).all()
    a = dst[:, :, 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    got, won = ms.merge_bgra(dst, src, False)
    assert np.array_equal(got, dst) and won == 0
    dst, src = ms.make_pair_bgra("specials", np.random.default_rng(4))
    got, won = ms.merge_bgra(dst, src, False)
    win = dst[:, :, 3].astype(int) < src[:, :, 3].astype(int)
    assert np.array_equal(got, np.where(win[:, :, None], src, dst)) and won == win.sum()
    assert ((dst[:, :, 3] == 127) & (src[:, :, 3] == 128)).any()         # a signed compare of the byte would lose these
    assert np.array_equal(ms.merge_bgra(dst, src, True)[0], src)


# ---------------------------------------------------------------- item counts
def test_item_counts_at_eight_bands():
    """int16: 8192 + 2048 + 512 + 128 + 32 + 8 + 2 groups of 8, then 4 + 1 pixels; fp32: 16384 + ... + 4 + 1 groups of 4, then 1 pixel.
    Levels 0 and 1 of int16 end on chunk boundaries (8 and 10 chunks of 1024 items), levels 2 .. 8 share the last block."""
    assert ms.item0(8, 0) == [0, 8192, 10240, 10752, 10880, 10912, 10920, 10922, 10926, 10927]
    assert ms.item0(8, 1)[-1] == 21846 and ms.item0(8, 1)[-3:] == [21844, 21845, 21846]
    assert ms.item0(8, 0)[1] % 1024 == 0 and ms.item0(8, 0)[2] % 1024 == 0 and -(-10927 // 1024) == 11 and -(-21846 // 1024) == 22
    assert [i for i in range(9) if ms.is_scalar_level(i, 0)] == [7, 8] and [i for i in range(9) if ms.is_scalar_level(i, 1)] == [8]
    assert ms.item0(0, 0) == [0, 8192] and ms.item0(0, 1) == [0, 16384]


# ---------------------------------------------------------------- path coverage of the multi-band cases
@pytest.mark.parametrize("bands,ff", ms.COMBOS)
def test_merge_cases_reach_every_path(bands, ff):
    cases = cases_of(bands, ff)
    gpx = ms.GPX[ff]
    kinds = [(c["kind"], c["pos"]) for c in cases]
    assert kinds[:-3] == ms.kind_list(bands, ff) and len({c["t"] for c in cases}) == len(cases) >= 10
    assert sum(c["dst"] is None for c in cases) == 2 and sum(c["src"] is None for c in cases) == 1
    lay = pi.slot_layout(bands, ff)
    for c in cases:
        for img, pad in ((c["dst"], ms.DST_PAD), (c["src"], ms.SRC_PAD)):
            assert img is None or (img.size == lay["total"] and (pi.padding_of(img, bands, ff) == pad).all())
    held = [c for c in cases if c["dst"] is not None and c["src"] is not None]
    wins = {(c["kind"], c["pos"]): level_wins(c, bands, ff) for c in held}
    mixed = [wins[("mixed", p)] for p in range(3)]
    for i in range(bands + 1):
        n = (256 >> i) ** 2
        if ms.is_scalar_level(i, ff):
            every = np.concatenate([m[i] for m in mixed])
            assert every.any() and not every.all(), i                    # the scalar tail wins and loses
        else:
            assert set().union(*(group_kinds(m[i], gpx) for m in mixed)) == {"all", "none", "part"}, i
            if n // gpx >= 3:
                assert all(group_kinds(m[i], gpx) == {"all", "none", "part"} for m in mixed), i
        for (kind, pos), w in wins.items():
            if kind == "lone_win":
                assert w[i].sum() == 1 and w[i][ms.lone_index(pos + i, n, gpx)], (kind, pos, i)
            elif kind == "lone_loss":
                assert (~w[i]).sum() == 1 and not w[i][ms.lone_index(pos + i, n, gpx)], (kind, pos, i)
            elif kind == "ties":
                assert w[i].all(), i
    # every lane pattern but "all" and "none" is met in the partly won groups of level 0, the all-but-lane-0 one among them
    part = np.concatenate([m[0].reshape(-1, gpx) for m in mixed])
    code = (part << np.arange(gpx)).sum(axis=1)
    assert set(code.tolist()) == set(range(1 << gpx)), bands
    # ties: bit-equal weights, and -0.0 / +0.0 both ways round, with Laplacians that differ
    c = next(c for c in held if c["kind"] == "ties")
    (dl, dw), (sl, sw) = pi.unpack(c["dst"], bands, ff), pi.unpack(c["src"], bands, ff)
    db, sb = dw[0].view(np.uint32), sw[0].view(np.uint32)
    assert ((db == sb) & (db & 0x7FFFFFFF != 0)).any() and ((db == 0x80000000) & (sb == 0)).any() and ((db == 0) & (sb == 0x80000000)).any()
    assert all(a.tobytes() != b.tobytes() for a, b in zip(dl, sl))
    # specials: every value against every value at level 0; NaN on either side never wins
    c = next(c for c in held if c["kind"] == "specials")
    dw, sw = pi.unpack(c["dst"], bands, ff)[1], pi.unpack(c["src"], bands, ff)[1]
    met = set(zip(dw[0].view(np.uint32).reshape(-1).tolist(), sw[0].view(np.uint32).reshape(-1).tolist()))
    assert len(met) == ms.SPECIALS.size ** 2
    w0 = wins[("specials", 0)][0]
    assert not w0[(np.isnan(dw[0]) | np.isnan(sw[0])).reshape(-1)].any() and w0.any() and not w0.all()
    if ff:
        bits = pi.unpack(held[0]["src"], bands, ff)[0][0].view(np.uint32)
        assert all((bits == b).any() for b in ms.LAP_SPECIALS.view(np.uint32)) and np.isnan(bits.view(np.float32)).mean() > 0.03


def test_lone_positions_cover_first_and_last_item_of_every_level():
    """at 8 bands the six tiles of a lone_* kind take, at every level, all six positions: index 0 and index n - 1 -- the first and the
    last item of the level -- are each a lone winner and a lone loser; the other band counts meet all six between them"""
    for ff in (0, 1):
        gpx = ms.GPX[ff]
        for kind in ("lone_win", "lone_loss"):
            ps = [p for k, p in ms.kind_list(8, ff) if k == kind]
            assert len(ps) == 6
            for i in range(9):
                n = (256 >> i) ** 2
                assert {ms.lone_index(p + i, n, gpx) for p in ps} == {min(max(v, 0), n - 1) for v in (0, 1, gpx - 1, gpx, n - gpx, n - 1)}
            rest = {p % 6 for b, f in ms.COMBOS if b != 8 for k, p in ms.kind_list(b, f) if k == kind}
            assert rest == set(range(6))
    assert [ms.lone_index(p, 65536, 8) for p in range(6)] == [0, 1, 7, 8, 65528, 65535]
    assert [ms.lone_index(p, 4, 8) for p in range(6)] == [0, 1, 3, 3, 0, 3] and ms.lone_index(5, 1, 4) == 0


# ---------------------------------------------------------------- the other case sets
def test_bgra_cases_reach_every_path():
    cases = ms.bgra_cases()
    wins = {}
    for c in cases:
        if c["dst"] is not None and c["src"] is not None:
            wins[(c["kind"], c["pos"])] = c["dst"].reshape(-1, 4)[:, 3] < c["src"].reshape(-1, 4)[:, 3]
    n = 256 * 256
    for p in range(3):
        assert group_kinds(wins[("mixed", p)], 4) == {"all", "none", "part"}
    assert set((np.concatenate([wins[("mixed", p)] for p in range(3)]).reshape(-1, 4) << np.arange(4)).sum(axis=1).tolist()) == set(range(16))
    for p in range(6):
        w, l = wins[("lone_win", p)], wins[("lone_loss", p)]
        assert w.sum() == 1 and w[ms.lone_index(p, n, 4)] and (~l).sum() == 1 and not l[ms.lone_index(p, n, 4)]
    assert not wins[("ties", 0)].any() and not wins[("ties_swapped", 0)].any()
    a, b = (next(c for c in cases if c["kind"] == k) for k in ("ties", "ties_swapped"))
    assert a["dst"].tobytes() == b["src"].tobytes() and a["src"].tobytes() == b["dst"].tobytes() and a["dst"].tobytes() != a["src"].tobytes()
    assert wins[("specials", 0)].any() and not wins[("specials", 0)].all()
    assert sum(c["dst"] is None for c in cases) == 2 and sum(c["src"] is None for c in cases) == 1
    assert all(c[k] is None or c[k].size == n * 4 for c in cases for k in ("dst", "src"))


def test_batch_cases_straddle_the_launch_batch():
    cases, images = ms.batch_cases()
    assert len(cases) == ms.MERGE_BATCH + 3 == 515 and len({c["t"] for c in cases}) == 515 and len(images) == 4
    assert len({im.tobytes() for im in images}) == 4 and all(im.size == 655360 for im in images)
    xs, ys = [c["t"][0] for c in cases], [c["t"][1] for c in cases]
    assert min(xs) == min(ys) == -11 and max(xs) == max(ys) == 11
    assert [c["t"] for c in cases] != sorted((c["t"] for c in cases), key=lambda t: t[::-1])        # not the store's order
    held = [k for k, c in enumerate(cases) if c["dst"] is not None]
    assert tuple(held) == ms.BATCH_HELD and len({cases[k]["dst"].tobytes() for k in held}) == 7
    assert [c["src"] for c in cases] == [k % 4 for k in range(515)]
    for k in held:
        c = dict(cases[k], src=images[cases[k]["src"]])
        assert group_kinds(level_wins(c, 0, 0)[0], 8) == {"all", "none", "part"}, k
    _, won, pairs, fresh = ms.expected(cases, images, 0, 0)
    assert (pairs, fresh) == (515, 508) and won > 0


def test_state_cases_straddle_the_staging_batch():
    first = ms.STAGE_BYTES // pi.slot_layout(8, 1)["total"]
    assert first == 23
    coords = [(x, y) for y in range(2) for x in range(13)]
    cases, b = ms.state_cases(coords)
    assert b == first and len(cases) == 26
    assert [k for k, c in enumerate(cases) if c["dst"] is not None] == [21, 22, 23, 24]
    assert {c["kind"] for c in cases} == {"mixed", "specials"} and all(c["kind"] == "mixed" for c in cases[21:25])
    for c in cases[21:25]:
        w = level_wins(c, 8, 1)
        assert group_kinds(w[0], 4) == {"all", "none", "part"}
    assert len({c["src"].tobytes() for c in cases}) == 26
