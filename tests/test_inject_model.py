"""The injected pyramids (pyramid_inject.py) without a GPU: the slot layout against totals worked out by hand, pack / unpack, and the
conditions the generators must meet to bite -- saturating collapses, 8U views inside the range, every tie of the fp32 view, weights
half zero.  These are conditions on the inputs of tests/test_gpu_inject.py, checked on the model alone."""
import numpy as np
import pytest

import pyramid_inject as pi
from map_model import to_8u

# slot sizes from the rule, by hand.  Laplacians then weights, every level rounded up to 256 bytes:
#   0 bands, 16S: 256^2*6 = 393216; 256^2*4 = 262144
#   5 bands, 16S: 393216 + 98304 + 24576 + 6144 + 1536 + (384 -> 512) = 524288; 262144 + 65536 + 16384 + 4096 + 1024 + 256 = 349440
#   8 bands, 32F: 786432 + 196608 + 49152 + 12288 + 3072 + 768 + (192, 48, 12 -> 256 each) = 1049088;
#                 262144 + 65536 + 16384 + 4096 + 1024 + 256 + (64, 16, 4 -> 256 each) = 350208
SLOT_BYTES = {(0, 0): 655360, (5, 0): 873728, (8, 1): 1399296}


def test_layout_totals_are_the_hand_computed_ones():
    for (bands, ff), total in SLOT_BYTES.items():
        lay = pi.slot_layout(bands, ff)
        assert lay["total"] == total and lay["nlev"] == bands + 1
        assert all(o % 256 == 0 for o in lay["lap_off"] + lay["w_off"]) and lay["lap_off"][0] == 0
    assert pi.slot_layout(11, 0) == pi.slot_layout(8, 0)                 # the band count is capped at log2(256)
    assert pi.slot_layout(5, 0)["w_off"][0] == 524288 and pi.slot_layout(8, 1)["w_off"][0] == 1049088


@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("bands", range(9))
def test_unpack_inverts_pack_and_the_padding_is_not_zero(bands, force_float):
    rng = np.random.default_rng([bands, force_float])
    lap = pi.make_lap("wide" if force_float else "full", force_float, bands, rng)
    w = pi.make_w("signs", bands, rng)
    buf = pi.pack(lap, w)
    assert buf.dtype == np.uint8 and buf.size == pi.slot_layout(bands, force_float)["total"]
    lap2, w2 = pi.unpack(buf, bands, force_float)
    assert len(lap2) == len(w2) == bands + 1
    for a, b in zip(lap + w, lap2 + w2):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()         # bytes: -0.0 stays -0.0
    pad = pi.padding_of(buf, bands, force_float)
    assert (pad == pi.PAD).all()
    # the first level that needs rounding: 8 x 8 of 16S (384 bytes), 4 x 4 of 32F (192 bytes; its weights take 64)
    assert (pad.size > 0) == (bands >= (6 if force_float else 5))


def test_generators_are_seeded_and_independent_per_level():
    a, _ = pi.make_tiles(5, 0, "nine", "full", "half", 3)
    b, _ = pi.make_tiles(5, 0, "nine", "full", "half", 3)
    c, _ = pi.make_tiles(5, 0, "nine", "full", "half", 4)
    t = pi.SHAPES["nine"][4]
    assert all(np.array_equal(x, y) for x, y in zip(a[t][0] + a[t][1], b[t][0] + b[t][1]))
    assert not np.array_equal(a[t][0][0], c[t][0][0])
    u = pi.SHAPES["nine"][5]
    assert not np.array_equal(a[t][0][0], a[u][0][0])
    # a level is not a shrunk copy of the one below it: the level-k zero set is its own
    assert not np.array_equal(a[t][1][1] == 0, a[t][1][0][::2, ::2] == 0)
    for shape, coords in pi.SHAPES.items():
        assert len(coords) == len(set(coords)) <= 10 and min(min(c) for c in coords) < 0, shape
    assert pi.lone_positions(0) == list(pi.LONE) and pi.lone_positions(8) == [(0, 0)]
    assert pi.lone_positions(3) == [(0, 0), (0, 31), (31, 0), (31, 31), (0, 3), (1, 4), (3, 0), (4, 0), (7, 15), (8, 16)]


def unmasked_blends(m):
    """the raw blends of every tile and the mask of their unmasked components"""
    raws, keep = [], []
    for t in m.tiles():
        raws.append(m.blend_tile_raw(*t))
        keep.append(np.broadcast_to((m.tiles_[t][1][0] != 0)[:, :, None], raws[-1].shape))
    return np.stack(raws), np.stack(keep)


@pytest.mark.parametrize("kind", ["rails", "full", "opposed"])
def test_int16_kinds_saturate_the_collapse(kind):
    tiles, _ = pi.make_tiles(5, 0, "nine", kind, "half", 1)
    m = pi.model_of(tiles, 5, 0)
    raw, keep = unmasked_blends(m)
    v = raw[keep]
    hi, lo = float((v == 32767).mean()), float((v == -32768).mean())
    assert hi + lo >= 0.02, (kind, hi, lo)
    if kind == "opposed":
        # both directions, in every pixel: the walk of the constant collapse goes over each rail once
        g, over = 32767, []
        for i in range(4, -1, -1):
            s = g + pi.opposed_value(i, 5)
            over.append((s > 32767) - (s < -32768))
            g = min(max(s, -32768), 32767)
        assert 1 in over and -1 in over and g == -32768 and (v == -32768).all()
    else:
        assert hi > 0 and lo > 0


@pytest.mark.parametrize("force_float", [0, 1])
def test_view_kinds_land_inside_the_8u_range(force_float):
    tiles, _ = pi.make_tiles(5, force_float, "nine", "view", "half", 2)
    m = pi.model_of(tiles, 5, force_float)
    raw, keep = unmasked_blends(m)
    v = to_8u(raw)[keep]
    assert float(((v >= 1) & (v <= 254)).mean()) >= 1 / 3
    assert (v == 0).any() and (v == 255).any()                          # and the clamp at both ends


def test_ties_hold_every_n_and_the_model_rounds_them_to_even():
    tab = pi.tie_values()
    assert sorted(tab) == list(range(-2, 258))
    for n, v in tab.items():
        assert v.dtype == np.float32 and np.float32(v) * np.float32(255) == np.float32(n + 0.5)
    for bands in (1, 8):
        tiles, _ = pi.make_tiles(bands, 1, "one", "ties", "half", 5)
        m = pi.model_of(tiles, bands, 1)
        (t,) = m.tiles()
        lap0, w0 = m.tiles_[t][0][0], m.tiles_[t][1][0]
        raw = m.blend_tile_raw(*t)
        keep = w0 != 0
        assert np.array_equal(raw[keep], lap0[keep])                     # upper levels zero: the collapse is lap_0, at any band count
        prod = (raw * np.float32(255))[keep]
        out = to_8u(raw)[keep]
        for n in range(256):
            at = prod == np.float32(n + 0.5)
            assert at.any(), n
            assert (out[at] == min(n + (n & 1), 255)).all(), n           # ties to even; 255.5 -> 256 saturates to 255
        assert (out[prod < 0] == 0).all() and (out[prod > 256] == 255).all() and (prod < -1).any() and (prod > 257).any()


def test_half_weights_are_about_half_zero_at_every_level():
    tiles, _ = pi.make_tiles(5, 0, "nine", "full", "half", 1)
    for i in range(6):
        z = np.concatenate([(w[i] == 0).reshape(-1) for _, w in tiles.values()])
        assert 0.3 <= float(z.mean()) <= 0.7, (i, float(z.mean()))


def test_weight_kinds_are_what_they_say():
    for kind in pi.W_KINDS:
        tiles, kinds = pi.make_tiles(5, 1, "holes", "wide", kind, 7)
        assert list(kinds.values()).count(kind) >= 5 and set(kinds.values()) <= {kind, "half"}
        seen = set()
        for t, (_, w) in tiles.items():
            if kinds[t] != kind or kind == "half":
                continue
            for i, a in enumerate(w):
                nz = a != 0
                if kind == "all":
                    assert nz.all()
                elif kind == "none":
                    assert not nz.any() and a.tobytes() == bytes(a.nbytes)
                elif kind == "lone_one":
                    assert int(nz.sum()) == 1 and tuple(np.argwhere(nz)[0]) in pi.lone_positions(i)
                elif kind == "lone_zero":
                    assert int((~nz).sum()) == 1 and tuple(np.argwhere(~nz)[0]) in pi.lone_positions(i)
                elif kind == "signs":
                    bits = a.view(np.uint32)
                    assert (bits == 0x80000000).any() and not nz[bits == 0x80000000].any()          # -0.0: zero
                    for b in (0x00000001, 0x80000001, 0x00800000):                                  # +-denormal, FLT_MIN: not zero
                        assert i > 3 or ((bits == b).any() and nz[bits == b].all())
                    assert i > 3 or ((a < -1e-30).any() and (a > 0.1).any())
                if kind.startswith("lone") and i == 0:
                    seen.add(tuple(np.argwhere(nz if kind == "lone_one" else ~nz)[0]))
        if kind.startswith("lone"):
            assert len(seen) == 5                                        # a position of its own for every such tile
    # seeds five apart cover all ten positions between them: what tests/test_gpu_inject.py gives the two pyramid types
    got = set()
    for seed in (7, 12):
        tiles, kinds = pi.make_tiles(5, 0, "holes", "full", "lone_one", seed)
        got |= {tuple(np.argwhere(w[0] != 0)[0]) for t, (_, w) in tiles.items() if kinds[t] == "lone_one"}
    assert got == set(pi.LONE)
