"""The feed-side select on slot images that no keyframe leaves behind, test code only: the byte-level rule of the level kernel's
max-weight select into the tiles (feed_slot; csrc/kernels.hip level3_block stage D, select_store, k_lap_select, strips.inc) and of the
single-band map's (feed_bgra; csrc/single_band.hip), and seeded generators of stored state built AROUND the keyframe's own weights --
one ulp either side of them, quad by quad, the values the kernels keep as sentinels -- for tests/test_feed_slots.py (CPU: the rule
against ModelMap / ModelMapSingleBand, and the conditions the generators must meet to bite) and tests/test_gpu_feed_slots.py (the
kernels against the rule, on whole exported slots).  The slot layout, pack / unpack and the tile RNG convention are pyramid_inject.py's,
the special values merge_slots.py's; neither is restated here.

The numbered gaps the generators' docstrings name:
  1 the comparison itself (tie, +1 ulp, -1 ulp, pixel by pixel at every level)      2 values no keyframe leaves, the kernels' own
  sentinels (NaN: culled, -1: fresh) among them      3 the 2 x 2 quad: its 16 win patterns, the small levels, the top level
  4 collateral writes: every byte the keyframe did not win      5 fresh and stored tiles in one launch      6 the band counts
  7 cull bounds that tile_import must forget      8 the kernel forms the product does not take

Nothing here needs a GPU to import."""
import numpy as np

import merge_slots as ms
import pyramid_inject as pi
from pyramid_inject import ELE

PAD = ms.DST_PAD                             # 0x3C: the padding of every image the map under test imports
KINDS = ("ties", "quads", "specials", "mixed", "lone_win", "lone_loss")
# the kinds in the order the imported tiles take them: the first three are ties at the small levels, so that the rotation by
# (tile index + level) meets all three classes there
CYCLE = ("ties", "quads", "ties", "specials", "mixed", "lone_win", "lone_loss")
TIE, ABOVE, BELOW = 0, 1, 2                  # the classes of `ties`: stored == kf_w (won), one ulp above it (lost), one ulp below (won)
SPECIAL_W = np.concatenate([ms.SPECIALS, np.array([-1.0], np.float32)])          # ... and the fresh-tile sentinel, stored
FLT_MAX = np.float32(3.4028234663852886e38)
F_INF = np.float32(np.inf)
BGRA_KINDS = ("ties", "specials")


# ---------------------------------------------------------------- the rule
def feed_slot(stored_lap, stored_w, kf_lap, kf_w, fresh):
    """([lap_0 .. lap_L], [w_0 .. w_L], won) of a tile after one keyframe.  Per level win = kf_w >= stored_w in float32 (NaN on either
    side: false); a fresh tile's pixels all win, whatever it holds.  Won pixels take the keyframe's three components and its weight as
    bit patterns, lost pixels keep theirs (through integer views: NaN payloads and -0.0 survive).  won counts the winning pixel-levels."""
    lap, w, won = [], [], 0
    for i in range(len(kf_w)):
        if fresh:
            win = np.ones(kf_w[i].shape, bool)
            ol, ow = np.empty_like(kf_lap[i]), np.empty_like(kf_w[i])
        else:
            with np.errstate(invalid="ignore"):
                win = kf_w[i] >= stored_w[i]
            ol, ow = stored_lap[i].copy(), stored_w[i].copy()
        ut = np.uint32 if kf_lap[i].dtype == np.float32 else np.uint16
        ow.view(np.uint32)[win] = kf_w[i].view(np.uint32)[win]
        ol.view(ut)[win] = kf_lap[i].view(ut)[win]
        lap.append(ol); w.append(ow)
        won += int(win.sum())
    return lap, w, won


def feed_bgra(stored, kf):
    """The single-band rule (csrc/single_band.hip, the last lines of k_single): a fresh tile (stored None) takes kf where kf's alpha is
    not 0 and 0 elsewhere; a stored tile takes kf where stored.a < kf.a, as unsigned bytes."""
    kf = np.asarray(kf, np.uint8).reshape(ELE, ELE, 4)
    if stored is None:
        out = kf.copy()
        out[kf[:, :, 3] == 0] = 0
        return out
    out = np.asarray(stored, np.uint8).reshape(ELE, ELE, 4).copy()
    win = out[:, :, 3] < kf[:, :, 3]
    out[win] = kf[win]
    return out


def wins_of(stored_w, kf_w):
    with np.errstate(invalid="ignore"):
        return np.asarray(kf_w, np.float32) >= np.asarray(stored_w, np.float32)


# ---------------------------------------------------------------- stored weights around the keyframe's
def tie_classes(kw, rot, rng):
    """the class of every pixel of one level: drawn in equal parts, or in rotation from `rot` where the level has fewer than 16 pixels"""
    if kw.size < 16:
        return ((rot + np.arange(kw.size)) % 3).reshape(kw.shape)
    return rng.integers(0, 3, kw.shape)


def around(kw, cls):
    return np.where(cls == TIE, kw, np.where(cls == ABOVE, np.nextafter(kw, F_INF), np.nextafter(kw, -F_INF))).astype(np.float32)


def class_of(stored_w, kf_w):
    """TIE / ABOVE / BELOW where the stored weight is the keyframe's or one ulp from it, -1 elsewhere"""
    out = np.full(kf_w.shape, -1)
    for c in (TIE, ABOVE, BELOW):
        out[around(kf_w, np.full(kf_w.shape, c)).view(np.uint32) == stored_w.view(np.uint32)] = c
    return out


def quad_patterns(win):
    """the 4-bit win pattern of every aligned 2 x 2 quad of a level: bit 2 * row + column"""
    q = win.astype(np.int64)
    return q[0::2, 0::2] | (q[0::2, 1::2] << 1) | (q[1::2, 0::2] << 2) | (q[1::2, 1::2] << 3)


def quad_weights(kw, rng):
    """gap 3: the 16 win patterns, one per aligned quad, in a seeded permutation over the level: kf_w wins, the next float above
    it loses"""
    h = kw.shape[0] // 2
    pat = rng.permutation(np.arange(h * h) % 16).reshape(h, h)
    win = np.empty(kw.shape, bool)
    for b in range(4):
        win[(b >> 1)::2, (b & 1)::2] = (pat >> b) & 1
    return around(kw, np.where(win, TIE, ABOVE))


def make_stored(kind, ff, kf_w, k, rng):
    """([lap_0 .. lap_L], [w_0 .. w_L]) of one imported tile; kf_w: the keyframe's own weights of that tile, k: the tile's index in
    the case (rotation of the small levels, position of the lone pixel), rng: the tile's own generator -- the Laplacians are drawn
    first, then the weights.
    ties      (gaps 1, 2)  every pixel the keyframe's weight, the float above it or the float below it; under a keyframe weight of
                           0 these are +-1e-45: the denormals must compare as IEEE values
    quads     (gap 3)      levels 0 and 1 quad_weights, the others ties
    specials  (gap 2)      `mixed` with an eighth of the pixels from SPECIAL_W: NaN of both signs (never won, their bytes stay),
                           +-inf, +-0, denormals, FLT_MAX, negative normals, and -1.0 exactly (won: the tile is not fresh)
    mixed                  pyramid_inject's "half": uniform in (0.01, 1), half of them zero
    lone_win  (gaps 3, 4)  FLT_MAX but for one 0 at lone_positions(level)[k]: one store in the whole level
    lone_loss (gaps 3, 4)  -1.0 but for one NaN there: one pixel of the level kept
    Laplacians: "full" int16, "wide" fp32; in the fp32 specials tile an eighth of the values are merge_slots.LAP_SPECIALS."""
    L = len(kf_w) - 1
    lap = pi.make_lap("wide" if ff else "full", ff, L, rng)
    if kind in ("mixed", "specials"):
        w = pi.make_w("half", L, rng)
    else:
        w = []
        for i, kw in enumerate(kf_w):
            if kind == "quads" and i < 2:
                a = quad_weights(kw, rng)
            elif kind in ("ties", "quads"):
                a = around(kw, tie_classes(kw, k + i, rng))
            elif kind in ("lone_win", "lone_loss"):
                ps = pi.lone_positions(i)
                a = np.full(kw.shape, FLT_MAX if kind == "lone_win" else -1.0, np.float32)
                a[ps[k % len(ps)]] = 0.0 if kind == "lone_win" else np.nan
            else:
                raise ValueError(kind)
            w.append(np.ascontiguousarray(a, np.float32))
    if kind == "specials":
        for i in range(L + 1):
            sp = rng.random(w[i].shape) < 0.125
            w[i][sp] = SPECIAL_W[rng.integers(0, SPECIAL_W.size, w[i].shape)][sp]
            if ff:
                sp = rng.random(lap[i].shape) < 0.125
                lap[i][sp] = ms.LAP_SPECIALS[rng.integers(0, ms.LAP_SPECIALS.size, lap[i].shape)][sp]
    return lap, w


# ---------------------------------------------------------------- the cases
def outside_of(canvas):
    """a coordinate off the canvas, diagonally behind its last tile"""
    return (max(t[0] for t in canvas) + 1, max(t[1] for t in canvas) + 1)


def make_rounds(kf, bands, ff, seed=300):
    """The case of one band count and type as a list of rounds, one map each: kf = {t: (lap, w)} is the keyframe's own pyramid on every
    tile of its canvas.  In every round all but one of the canvas' tiles are imported, taking CYCLE's kinds in turn with an index k
    that runs on through the rounds; the remaining tile stays fresh (gap 5; another one every round) and a `specials` tile off the
    canvas is imported too.  There are as many rounds as it takes k to go through CYCLE once -- one for a canvas of eight tiles or
    more, three for 2 x 2 -- and every round has a seed of its own: [seed + round, j, bands, ff] is tile j's RNG stream, in
    pyramid_inject's convention.  A round is {"fresh": t, "outside": t, "kinds": {t: (kind, k)}, "stored": {t: (lap, w)}}."""
    canvas = sorted(kf, key=lambda t: t[::-1])
    assert len(canvas) >= 2
    n = len(canvas) - 1
    rounds, k = [], 0
    for r in range(-(-len(CYCLE) // n)):
        fresh = canvas[(r + bands) % len(canvas)]
        rd = {"fresh": fresh, "outside": outside_of(canvas), "kinds": {}, "stored": {}}
        held = [t for t in canvas if t != fresh]
        for j, t in enumerate(held + [rd["outside"]]):
            rng = np.random.default_rng([seed + r, j, bands, int(bool(ff))])
            kind = CYCLE[k % len(CYCLE)] if t in kf else "specials"
            kw = kf[t][1] if t in kf else [np.zeros((ELE >> i, ELE >> i), np.float32) for i in range(min(bands, 8) + 1)]
            rd["kinds"][t] = (kind, k)
            rd["stored"][t] = make_stored(kind, ff, kw, k, rng)
            k += t in kf
        rounds.append(rd)
    return rounds


def expected_round(rd, kf):
    """({t: (lap, w)} after the keyframe, pixel-levels won on tiles that were not fresh): feed_slot on every tile of the canvas, the
    tile off the canvas as it was imported"""
    out, won = {}, 0
    for t in set(kf) | set(rd["stored"]):
        if t not in kf:
            out[t] = rd["stored"][t]
        elif t in rd["stored"]:
            lap, w, n = feed_slot(rd["stored"][t][0], rd["stored"][t][1], kf[t][0], kf[t][1], False)
            out[t] = (lap, w)
            won += n
        else:
            out[t] = feed_slot(None, None, kf[t][0], kf[t][1], True)[:2]
    return out, won


def feed_tiles(state, kf):
    """a further keyframe over {t: (lap, w)}: tiles it does not hold are fresh"""
    out = dict(state)
    for t in kf:
        s = state.get(t)
        out[t] = feed_slot(s[0] if s else None, s[1] if s else None, kf[t][0], kf[t][1], s is None)[:2]
    return out


def check_bite(rounds, kf):
    """The conditions under which the case closes its gaps, on the weights of the keyframe as they were read back:
      every `ties` class on a pixel with kf_w > 0, at every level that has such a pixel (gap 1; the top level of 8 bands is one pixel);
      all 16 quad patterns at level 0 and at level 1 (gap 3);      every value of SPECIAL_W stored at level 0, on the canvas (gap 2);
      a win and a loss at every level (gaps 1, 4);      one store / one kept pixel in every level of the lone_* tiles."""
    nlev = len(next(iter(kf.values()))[1])
    kinds = set()
    for i in range(nlev):
        classes, wins, some_kf = set(), set(), False
        pats = set()
        for rd in rounds:
            for t, (kind, _) in rd["kinds"].items():
                if t not in kf:
                    continue
                kinds.add(kind)
                sw, kw = rd["stored"][t][1][i], kf[t][1][i]
                win = wins_of(sw, kw)
                wins |= set(np.unique(win).tolist())
                some_kf = some_kf or bool((kw > 0).any())
                if kind == "ties" or (kind == "quads" and i >= 2):
                    classes |= set(class_of(sw, kw)[kw > 0].tolist())
                if kind == "quads" and i < 2:
                    pats |= set(quad_patterns(win).reshape(-1).tolist())
                if kind == "lone_win":
                    assert int(win.sum()) == 1, (t, i)
                if kind == "lone_loss":
                    assert int((~win).sum()) == 1 and np.isnan(sw[~win]).all(), (t, i)
                if kind == "specials" and i == 0:
                    bits = set(sw.view(np.uint32).reshape(-1).tolist())
                    assert all(int(b) in bits for b in SPECIAL_W.view(np.uint32)), t
                    assert not win[np.isnan(sw)].any() and win[sw == -1.0].all()
        assert wins == {True, False}, i
        assert not some_kf or classes == {TIE, ABOVE, BELOW}, (i, classes)
        assert i >= 2 or pats == set(range(16)), (i, sorted(pats))
    assert kinds == set(KINDS), kinds
    assert all(rd["fresh"] in kf and rd["outside"] not in kf for rd in rounds)


# ---------------------------------------------------------------- single band
def make_bgra(kind, kf, rng):
    """a stored single-band tile, random colour bytes.  ties: the keyframe's alpha, one above it or one below it (within the byte);
    specials: merge_slots.ALPHA_SPECIALS -- 0, 255 and both sides of the sign bit of a byte"""
    kf = np.asarray(kf, np.uint8).reshape(ELE, ELE, 4)
    out = rng.integers(0, 256, (ELE, ELE, 4)).astype(np.uint8)
    if kind == "ties":
        a = np.clip(kf[:, :, 3].astype(np.int64) + rng.integers(-1, 2, (ELE, ELE)), 0, 255)
    elif kind == "specials":
        a = ms.ALPHA_SPECIALS[rng.integers(0, ms.ALPHA_SPECIALS.size, (ELE, ELE))]
    else:
        raise ValueError(kind)
    out[:, :, 3] = a
    return out


def make_bgra_case(kf, seed=310):
    """{t: stored tile or None (fresh)} over the canvas of kf = {t: the keyframe alone}: the last tile fresh, the others `ties` and
    `specials` in turn; and a `specials` tile off the canvas"""
    canvas = sorted(kf, key=lambda t: t[::-1])
    assert len(canvas) >= 3
    stored = {}
    for j, t in enumerate(canvas[:-1] + [outside_of(canvas)]):
        rng = np.random.default_rng([seed, j, 0, 2])
        stored[t] = make_bgra(BGRA_KINDS[j % 2] if t in kf else "specials", kf.get(t, np.zeros((ELE, ELE, 4), np.uint8)), rng)
    stored[canvas[-1]] = None
    return stored


def expected_bgra(stored, kf):
    return {t: feed_bgra(s, kf[t]) if t in kf else s for t, s in stored.items()}


def check_bite_bgra(stored, kf):
    """an equal alpha above 0 with other colours, one above and one below the keyframe's, 127 against 128 (a signed compare of the
    byte would lose it), a fresh tile"""
    eq = up = down = sign = 0
    for t, s in stored.items():
        if s is None or t not in kf:
            continue
        sa, ka = s[:, :, 3].astype(int), kf[t][:, :, 3].astype(int)
        eq += int(((sa == ka) & (ka > 0) & (s[:, :, :3] != kf[t][:, :, :3]).any(axis=2)).sum())
        up += int((sa == ka + 1).sum()); down += int(((sa == ka - 1) & (ka > 0)).sum())
        sign += int(((sa <= 127) & (ka >= 128)).sum())
    assert eq and up and down and sign, (eq, up, down, sign)
    assert any(s is None for s in stored.values()) and any(t not in kf for t in stored)


# ---------------------------------------------------------------- the rig (these need the oracle or the library)
def rig(bands):
    """(prepare poses, [pose of keyframe 0, of keyframe 1], [keyframe 0, keyframe 1]) of tests/test_gpu_model.py's rig: the grid comes
    from both poses, so neither keyframe moves it"""
    from helpers import hostile_frame
    from test_gpu_model import COLS, ROWS, lattice_poses
    poses = lattice_poses(11 + bands)[:2]
    return poses, poses, [hostile_frame("noise", ROWS, COLS, k) for k in (0, 1)]


def copy_tiles(tiles):
    return {t: ([a.copy() for a in lw[0]], [a.copy() for a in lw[1]]) for t, lw in tiles.items()}
