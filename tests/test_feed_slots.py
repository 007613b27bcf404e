"""The byte-level rule of the feed-side select and its generators (feed_slots.py) without a GPU; no HIP code runs here.  The rule is
tied to the independent model once per band count and type -- ModelMap.tiles_ holds the generated stored state, the keyframe is fed
through feed_with_model, and every level of every tile equals feed_slot on the bit patterns -- so that tests/test_gpu_feed_slots.py
needs the rule alone.  The rest are conditions on that file's inputs, for exactly the rig and the parameters it uses: a generator that
stops reaching one of the places the cases are there for fails here."""
import functools

import numpy as np
import pytest

import feed_slots as fs
import merge_slots as ms
import pyramid_inject as pi
from helpers import feed_single_with_model, feed_with_model, workloads
from map_model import ModelMap, ModelMapSingleBand

BG = pi.BG


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def fed_model(bands, ff, k, tiles=None):
    """ModelMap holding `tiles`, fed keyframe k of the rig (the oracle gives the geometry of the feed)"""
    from oracle import orc
    from test_gpu_model import CAM
    prep, poses, frames = fs.rig(bands)
    o = orc.OracleMap(band_num=bands, force_float=ff, bg_color=BG)
    m = ModelMap(band_num=bands, force_float=ff, bg_color=BG)
    assert o.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    m.tiles_ = fs.copy_tiles(tiles or {})
    with np.errstate(invalid="ignore"):                                  # NaN weights: the model's `>=` is false on them, as IEEE has it
        assert feed_with_model(o, m, frames[k], poses[k])
    return m


@functools.lru_cache(maxsize=None)
def keyframe_of(bands, ff, k=0):
    return fed_model(bands, ff, k).tiles_


@functools.lru_cache(maxsize=None)
def rounds_of(bands, ff):
    return fs.make_rounds(keyframe_of(bands, ff), bands, ff)


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for t in want:
        for i, (gl, gw, wl, ww) in enumerate(zip(*got[t], *want[t])):
            assert gl.dtype == wl.dtype and np.array_equal(bits(gl), bits(wl)), ("lap", t, i)
            assert np.array_equal(bits(gw), bits(ww)), ("weight", t, i)


# ---------------------------------------------------------------- the rule against the models
@pytest.mark.parametrize("bands,ff", ms.COMBOS)
def test_rule_equals_the_model_on_every_round(orc, bands, ff):
    """every value of SPECIAL_W has a defined answer in numpy's `>=`, so none is taken out: NaN compares false on either side, -0.0
    equals 0.0, the denormals are ordered"""
    kf = keyframe_of(bands, ff)
    assert 4 <= len(kf) <= 9 and len(next(iter(kf.values()))[1]) == bands + 1
    seen = 0
    for rd in rounds_of(bands, ff):
        m = fed_model(bands, ff, 0, rd["stored"])
        want, won = fs.expected_round(rd, kf)
        assert_same(m.tiles_, want)
        total = sum(a.size for t in rd["stored"] if t in kf for a in kf[t][1])
        assert 0 < won < total
        # a stored NaN is never won and keeps its bytes; a stored -1.0 in a tile that is not fresh is won
        for t in (t for t, (kind, _) in rd["kinds"].items() if kind in ("specials", "lone_loss") and t in kf):
            sw, gw = rd["stored"][t][1][0], m.tiles_[t][1][0]
            nan, m1 = np.isnan(sw), sw == -1.0
            assert nan.any() and m1.any() and np.array_equal(bits(gw)[nan], bits(sw)[nan]) and np.array_equal(bits(gw)[m1], bits(kf[t][1][0])[m1])
            assert np.array_equal(bits(m.tiles_[t][0][0])[nan], bits(rd["stored"][t][0][0])[nan])
            seen += 1
    assert seen >= 2


@pytest.mark.parametrize("ff", [0, 1])
def test_rule_twice_equals_the_model_fed_two_keyframes(orc, ff):
    bands = 5
    kf, kf2 = keyframe_of(bands, ff), keyframe_of(bands, ff, 1)
    assert set(kf) != set(kf2) and set(kf) & set(kf2)                    # the second canvas shares tiles with the first and adds some
    rd = rounds_of(bands, ff)[0]
    m = fed_model(bands, ff, 0, rd["stored"])
    m2 = fed_model(bands, ff, 1, m.tiles_)
    assert_same(m2.tiles_, fs.feed_tiles(fs.expected_round(rd, kf)[0], kf2))


def single_band_fed(k, tiles=None):
    from oracle import orc
    from test_gpu_model import CAM, COLS, ROWS, lattice_poses
    from helpers import hostile_frame
    poses = lattice_poses(11)
    o = orc.OracleMap(single_band=1)
    m = ModelMapSingleBand()
    assert o.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    m.tiles_ = {t: a.copy() for t, a in (tiles or {}).items() if a is not None}
    assert feed_single_with_model(o, m, hostile_frame("noise", ROWS, COLS, k), poses[k])
    return m.tiles_


def test_bgra_rule_equals_the_single_band_model(orc):
    kf = single_band_fed(0)
    stored = fs.make_bgra_case(kf)
    fs.check_bite_bgra(stored, kf)
    got, want = single_band_fed(0, stored), fs.expected_bgra(stored, kf)
    assert sorted(got) == sorted(want)
    for t in want:
        assert np.array_equal(got[t], want[t]), t
    # the keyframe alone is the rule on a fresh tile; an equal alpha keeps the stored colours
    assert all(np.array_equal(fs.feed_bgra(None, kf[t]), kf[t]) for t in kf)
    t = next(t for t, s in stored.items() if s is not None and t in kf)
    eq = (stored[t][:, :, 3] == kf[t][:, :, 3]) & (kf[t][:, :, 3] > 0)
    assert eq.any() and np.array_equal(want[t][eq], stored[t][eq]) and not np.array_equal(want[t][eq], kf[t][eq])


# ---------------------------------------------------------------- the generators bite
@pytest.mark.parametrize("bands,ff", ms.COMBOS)
def test_generators_bite_on_the_rig(orc, bands, ff):
    kf, rounds = keyframe_of(bands, ff), rounds_of(bands, ff)
    fs.check_bite(rounds, kf)
    assert sum(len(rd["kinds"]) - 1 for rd in rounds) >= len(fs.CYCLE)
    lay = pi.slot_layout(bands, ff)
    for rd in rounds:
        for t, (lap, w) in rd["stored"].items():
            img = pi.pack(lap, w, pad=fs.PAD)
            assert img.size == lay["total"] and (pi.padding_of(img, bands, ff) == fs.PAD).all()
            if ff and rd["kinds"][t][0] == "specials":
                assert all((bits(lap[0]) == b).any() for b in bits(ms.LAP_SPECIALS))
    if bands == 8:
        # the top level is one pixel: the three ties-like tiles of the cycle hold the three classes there, over a keyframe weight > 0
        top = {int(fs.class_of(rd["stored"][t][1][8], kf[t][1][8])[0, 0]) for rd in rounds for t, (kind, _) in rd["kinds"].items()
               if kind in ("ties", "quads") and kf[t][1][8][0, 0] > 0}
        assert top == {fs.TIE, fs.ABOVE, fs.BELOW}


def test_rule_and_generators_on_made_up_weights():
    """the pieces on their own, without a model: patterns, classes, denormals under a zero keyframe weight, seeds"""
    rng = np.random.default_rng(1)
    kw = [rng.uniform(0, 1, (256 >> i, 256 >> i)).astype(np.float32) for i in range(9)]
    kw[0][:64] = 0
    for i in (0, 1):
        w = fs.quad_weights(kw[i], np.random.default_rng(2))
        pats = fs.quad_patterns(fs.wins_of(w, kw[i]))
        assert set(pats.reshape(-1).tolist()) == set(range(16))
        assert len({int(p) for p in (pats[0, 0], pats[0, -1], pats[-1, 0], pats[-1, -1])}) >= 2
    lap, w = fs.make_stored("ties", 1, kw, 4, np.random.default_rng(3))
    c = fs.class_of(w[0], kw[0])
    assert (c >= 0).all() and all(abs(float((c == k).mean()) - 1 / 3) < 0.02 for k in range(3))
    zero = kw[0] == 0
    assert set(bits(w[0])[zero].tolist()) == {0, 1, 0x80000001}                 # 0, 1e-45, -1e-45
    win = fs.wins_of(w[0], kw[0])
    assert win[zero & (bits(w[0]) == 0x80000001)].all() and not win[zero & (bits(w[0]) == 1)].any()
    assert [int(fs.class_of(w[i], kw[i])[0, 0]) for i in (7, 8)] == [(4 + 7) % 3, (4 + 8) % 3]
    klap = [np.zeros((256 >> i, 256 >> i, 3), np.float32) for i in range(9)]
    ol, ow, won = fs.feed_slot(lap, w, klap, kw, False)
    assert won == sum(int(fs.wins_of(a, b).sum()) for a, b in zip(w, kw))
    lost = ~win
    assert np.array_equal(bits(ow[0])[lost], bits(w[0])[lost]) and np.array_equal(bits(ol[0])[lost], bits(lap[0])[lost])
    assert (ol[0][win] == 0).all() and np.array_equal(ow[0][win], kw[0][win])
    fl, fw, n = fs.feed_slot(None, None, klap, kw, True)
    assert n == sum(a.size for a in kw) and all(np.array_equal(a, b) for a, b in zip(fw, kw))
    again = fs.make_stored("ties", 1, kw, 4, np.random.default_rng(3))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lap + w, again[0] + again[1]))
    for kind, n_won in (("lone_win", 1), ("lone_loss", None)):
        _, w = fs.make_stored(kind, 0, kw, 3, np.random.default_rng(4))
        for i in range(9):
            win = fs.wins_of(w[i], kw[i])
            ps = pi.lone_positions(i)
            assert (int(win.sum()) == 1 and win[ps[3 % len(ps)]]) if n_won else (int((~win).sum()) == 1 and not win[ps[3 % len(ps)]])
