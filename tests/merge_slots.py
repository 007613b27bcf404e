"""The map merge on slot images that no keyframe leaves behind, test code only: a byte-level model of csrc/merge.hip's rule on packed
slots (merge_slot, merge_bgra) and seeded generators of (dst, src) pairs for tests/test_merge_slots.py (CPU: the model against the
oracle, and the conditions the generators must meet to bite) and tests/test_gpu_merge_slots.py (the kernels against the model, on
bytes).  The slot layout, pack / unpack and the tile RNG convention are pyramid_inject.py's; nothing is restated here but the count of
the kernel's items, which the lone_* positions are chosen for.

The numbered gaps the generators' docstrings name:
  1 the scalar tail (levels smaller than one group)     2 the item-to-level table (first and last item of every level)
  3 the partially won group                             4 the comparison on values no keyframe leaves
  5 bytes that belong to no level                       6 more than kMergeBatch = 512 pairs
  7 the `won` counter                                   8 more than one staging batch of state-file records

Nothing here needs a GPU to import."""
import numpy as np

from pyramid_inject import ELE, pack, slot_layout, unpack

GPX = {0: 8, 1: 4}                           # pixels of one vector item: two 16-byte vectors of weights for int16 pyramids, one for fp32
BGRA_GPX = 4
DST_PAD, SRC_PAD = 0x3C, 0xA5                # padding of the images dst holds / of the images merged into it
GUARD, GUARD_BYTE = 64, 0x5A                 # bytes around every src image on the device
W_KINDS = ("mixed", "lone_win", "lone_loss", "ties", "specials")
BANDS = (0, 1, 2, 5, 7, 8)
COMBOS = [(bands, ff) for bands in BANDS for ff in (0, 1)]
MERGE_BATCH = 512                            # kMergeBatch of csrc/merge.hpp
STAGE_BYTES = 32 << 20                       # OutRing::kSlot: the state-file records of one staging batch


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


# NaN, -NaN, +inf, -inf, 0, -0.0, 1e-45, -1e-45, FLT_MIN, FLT_MAX, -0.75, 0.5
SPECIALS = _f32([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x7F7FFFFF,
                 0xBF400000, 0x3F000000])
ALPHA_SPECIALS = np.array([0, 1, 127, 128, 254, 255], np.uint8)         # the ends, and both sides of the sign bit of a byte
# what random bit patterns rarely hold in a small level: quiet and signalling NaNs with payloads, +-inf, -0.0
LAP_SPECIALS = _f32([0x7FC00000, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000])


# ---------------------------------------------------------------- the kernel's items, restated
def level_items(level, ff):
    """items of one level: a group of GPX pixels each, or one pixel each where the level is smaller than a group"""
    n = (ELE >> level) ** 2
    return n // GPX[ff] if n >= GPX[ff] else n


def item0(bands, ff):
    """first item of every level and, last, the items of a slot (MergePlan::item0)"""
    out = [0]
    for i in range(slot_layout(bands, ff)["nlev"]):
        out.append(out[-1] + level_items(i, ff))
    return out


def is_scalar_level(level, ff):
    return (ELE >> level) ** 2 < GPX[ff]


# ---------------------------------------------------------------- the model
def padding_mask(bands, ff):
    """True at the bytes of a slot image that belong to no level (what padding_of reads)"""
    zeros = np.zeros(slot_layout(bands, ff)["total"], np.uint8)
    return pack(*unpack(zeros, bands, ff), pad=1) == 1


def merge_slot(dst_bytes, src_bytes, bands, ff, dst_was_fresh):
    """(bytes, won) of dst's slot after src's was merged into it.  Fresh: src's image, every byte, won = 0.  Otherwise per level
    win = src_w >= dst_w in float32 (NaN on either side: false), Laplacians and weights move as bit patterns where win holds (through
    integer views: NaN payloads and -0.0 survive), every other byte of dst stays, padding included; won counts the winning
    pixel-levels."""
    d, s = (np.asarray(b, np.uint8).reshape(-1) for b in (dst_bytes, src_bytes))
    if dst_was_fresh:
        assert s.size == slot_layout(bands, ff)["total"]
        return s.copy(), 0
    (dl, dw), (sl, sw) = unpack(d, bands, ff), unpack(s, bands, ff)
    ut, won = np.uint32 if ff else np.uint16, 0
    for i in range(len(dw)):
        with np.errstate(invalid="ignore"):
            win = sw[i] >= dw[i]
        dw[i].view(np.uint32)[win] = sw[i].view(np.uint32)[win]
        dl[i].view(ut)[win] = sl[i].view(ut)[win]
        won += int(win.sum())
    out, pad = pack(dl, dw, pad=0), padding_mask(bands, ff)
    out[pad] = d[pad]
    return out, won


def merge_bgra(dst, src, dst_was_fresh):
    """the same for the single band's 256 x 256 x 4 uint8 slot: a pixel moves where dst's alpha is below src's"""
    d, s = (np.asarray(b, np.uint8).reshape(ELE, ELE, 4) for b in (dst, src))
    if dst_was_fresh:
        return s.copy(), 0
    win = d[:, :, 3] < s[:, :, 3]
    out = d.copy()
    out[win] = s[win]
    return out, int(win.sum())


def wins_of(dst_w, src_w):
    """the flat win mask of one level's weights, as the model takes it"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(src_w, np.float32) >= np.asarray(dst_w, np.float32)).reshape(-1)


# ---------------------------------------------------------------- win patterns
def lone_index(pos, n, gpx):
    """flattened index of a lone pixel: position pos (mod 6) of 0, 1, GPX-1, GPX, n-GPX, n-1, clamped into the level -- the first and
    last lane of the first group, the first lane of the second, the first and last lane of the last"""
    return min(max((0, 1, gpx - 1, gpx, n - gpx, n - 1)[pos % 6], 0), n - 1)


def mixed_wins(n, gpx, phase, rng):
    """the `mixed` pattern of one level of n pixels: group g is of kind (g + phase) % 3 -- all won, none won, won at a random non-empty
    proper subset of its lanes -- and the kinds are shuffled over the level where it has three groups or more (a level of one or two
    groups meets every kind over three phases).  In a scalar level pixel p wins when p + phase is odd."""
    if n < gpx:
        return (np.arange(n) + phase) % 2 == 1
    groups = n // gpx
    kinds = (np.arange(groups) + phase) % 3
    if groups >= 3:
        kinds = rng.permutation(kinds)
    win = np.zeros((groups, gpx), bool)
    win[kinds == 0] = True
    part = np.flatnonzero(kinds == 2)
    masks = rng.integers(1, (1 << gpx) - 1, part.size)                  # 1 .. 2^gpx - 2: not empty, not all
    win[part] = (masks[:, None] >> np.arange(gpx)) & 1
    return win.reshape(-1)


def lone_wins(kind, n, gpx, pos):
    win = np.zeros(n, bool) if kind == "lone_win" else np.ones(n, bool)
    win[lone_index(pos, n, gpx)] = kind == "lone_win"
    return win


def _positive(rng, n):
    return rng.uniform(0.01, 1.0, n).astype(np.float32)


def _other_side(w, above, rng):
    """weights on the given side of w (all positive): half of them one ulp away, half at twice / half the value"""
    near = np.nextafter(w, np.where(above, np.float32(4), np.float32(0)).astype(np.float32))
    far = (w * np.where(above, np.float32(2), np.float32(0.5))).astype(np.float32)
    return np.where(rng.random(w.size) < 0.5, near, far).astype(np.float32)


# ---------------------------------------------------------------- multi-band pairs
def make_lap(ff, bands, rng):
    """[lap_0 .. lap_L]: full-range int16, or fp32 from random bit patterns with an eighth of LAP_SPECIALS (NaN payloads, +-inf, -0.0);
    every pixel and channel on its own, so a swapped channel or half shows"""
    out = []
    for i in range(bands + 1):
        shp = (ELE >> i, ELE >> i, 3)
        if not ff:
            a = rng.integers(-32768, 32768, shp).astype(np.int16)
        else:
            a = rng.integers(0, 1 << 32, shp, dtype=np.uint64).astype(np.uint32).view(np.float32)
            sp = rng.random(shp) < 0.125
            a[sp] = LAP_SPECIALS[rng.integers(0, LAP_SPECIALS.size, shp)][sp]
        out.append(np.ascontiguousarray(a))
    return out


def make_pair(kind, bands, ff, rng, pos=0, src=None):
    """(dst, src) pyramids of one tile, each ([lap_0 .. lap_L], [w_0 .. w_L]); rng is the tile's own generator.
    mixed     (gaps 1, 3, 7)  mixed_wins with phase pos; src: a pyramid to derive dst from instead of drawing one (mixed only)
    lone_win  (gaps 1, 2, 3)  src wins exactly one pixel of level i, at lone_index(pos + i): every level has its own position
    lone_loss (gaps 2, 3)     src wins all but that pixel
    ties      (gap 4)         src_w == dst_w bit for bit on about half the pixels, -0.0 against +0.0 and +0.0 against -0.0 on the rest:
                              src wins everywhere, and dst must end with src's bits
    specials  (gap 4)         both weights drawn from SPECIALS, independently
    In mixed and lone_* the weights are positive, src's one ulp from dst's or at twice / half of it."""
    L, gpx = min(max(bands, 0), 8), GPX[int(bool(ff))]
    assert src is None or kind == "mixed"
    slap, sws = src if src is not None else (make_lap(ff, L, rng), None)
    dlap = make_lap(ff, L, rng)
    dws, out_sws = [], []
    for i in range(L + 1):
        s = ELE >> i
        n = s * s
        if kind in ("mixed", "lone_win", "lone_loss"):
            win = mixed_wins(n, gpx, pos, rng) if kind == "mixed" else lone_wins(kind, n, gpx, pos + i)
            sw = sws[i].reshape(-1) if sws is not None else _positive(rng, n)
            dw = _other_side(sw, ~win, rng)                               # src wins where dst lies below it
        elif kind == "ties":
            dw = np.where(rng.random(n) < 0.25, -1, 1).astype(np.float32) * _positive(rng, n)
            sw = dw.copy()
            zero = np.flatnonzero(rng.random(n) < 0.5)
            dw[zero] = np.where(np.arange(zero.size) % 2 == 0, np.float32(-0.0), np.float32(0.0))
            sw[zero] = -dw[zero]
        elif kind == "specials":
            dw, sw = SPECIALS[rng.integers(0, SPECIALS.size, n)], SPECIALS[rng.integers(0, SPECIALS.size, n)]
        else:
            raise ValueError(kind)
        dws.append(np.ascontiguousarray(dw, np.float32).reshape(s, s))
        out_sws.append(np.ascontiguousarray(sw, np.float32).reshape(s, s))
    return (dlap, dws), (slap, out_sws)


# ---------------------------------------------------------------- single-band pairs
def make_pair_bgra(kind, rng, pos=0):
    """(dst, src) of one single-band tile, 256 x 256 x 4 uint8, random colour bytes; the kinds of make_pair on the alpha byte, a group
    being 4 pixels.  ties (gap 4): equal alphas, 0 against 0 and 255 against 255 among them, with every colour byte different -- dst
    keeps its own.  specials: both alphas from ALPHA_SPECIALS."""
    n = ELE * ELE
    dst, src = (rng.integers(0, 256, (n, 4)).astype(np.uint8) for _ in range(2))
    if kind in ("mixed", "lone_win", "lone_loss"):
        win = mixed_wins(n, BGRA_GPX, pos, rng) if kind == "mixed" else lone_wins(kind, n, BGRA_GPX, pos)
        da = rng.integers(1, 255, n)
        near = rng.random(n) < 0.5
        sa = np.where(win, np.where(near, da + 1, rng.integers(da + 1, 256)), np.where(near, da - 1, rng.integers(0, da)))
    elif kind == "ties":
        da = rng.integers(0, 256, n)
        da[0::3] = 0; da[1::3] = 255
        sa = da
        src[:, :3] = dst[:, :3] ^ rng.integers(1, 256, (n, 3)).astype(np.uint8)
    elif kind == "specials":
        da, sa = ALPHA_SPECIALS[rng.integers(0, 6, n)], ALPHA_SPECIALS[rng.integers(0, 6, n)]
    else:
        raise ValueError(kind)
    dst[:, 3] = da; src[:, 3] = sa
    return dst.reshape(ELE, ELE, 4), src.reshape(ELE, ELE, 4)


# ---------------------------------------------------------------- the cases of the GPU tests
def _coord(j):
    return (j % 5 - 2, j // 5 - 1)


def _case(t, kind, pos, dst, src):
    return {"t": t, "kind": kind, "pos": pos, "dst": dst, "src": src}


def kind_list(bands, ff):
    """(kind, pos) of the tiles dst already holds in the merge of one band count and type: three phases of mixed, lone_win and
    lone_loss at all six positions at 8 bands and at one position elsewhere (2 * bands + ff, so the band counts rotate through
    them; lone_loss three further), ties, specials"""
    lone = range(6) if bands == 8 else [2 * bands + ff]
    return ([("mixed", p) for p in range(3)] + [("lone_win", p) for p in lone] + [("lone_loss", p + 3) for p in lone]
            + [("ties", 0), ("specials", 0)])


def merge_cases(bands, ff):
    """The tiles of one merge, gaps 1 - 5 and 7: every (kind, pos) of kind_list as a tile both maps hold, two tiles only src holds
    (fresh: copied whole, padding included) and one only dst holds (no src: it must come back untouched).  Every case is
    {"t", "kind", "pos", "dst", "src"} with packed images (None: that map does not hold the tile), dst's padded with 0x3C, src's
    with 0xA5; "pair" keeps the pyramids of the tiles both hold.  One RNG stream per tile, in pyramid_inject's convention."""
    seed = 100 + 2 * bands + ff
    plan = kind_list(bands, ff) + [("fresh", 1), ("fresh_specials", 0), ("dst_only", 0)]
    out = []
    for j, (kind, pos) in enumerate(plan):
        rng = np.random.default_rng([seed, j, bands, int(bool(ff))])
        gen = {"fresh": "mixed", "fresh_specials": "specials", "dst_only": "specials"}.get(kind, kind)
        dst, src = make_pair(gen, bands, ff, rng, pos)
        c = _case(_coord(j), kind, pos, pack(*dst, pad=DST_PAD), pack(*src, pad=SRC_PAD))
        if kind.startswith("fresh"):
            c["dst"] = None
        elif kind == "dst_only":
            c["src"] = None
        else:
            c["pair"] = (dst, src)
        out.append(c)
    return out


def bgra_cases():
    """the single band's merge (k_merge_bgra; gaps 3, 4, 5 and 7): the kinds of make_pair_bgra, ties in both directions (the second with dst and src exchanged), two
    fresh tiles and one only dst holds; images as flat bytes"""
    plan = [("mixed", p) for p in range(3)] + [("lone_win", p) for p in range(6)] + [("lone_loss", p) for p in range(6)]
    plan += [("ties", 0), ("ties_swapped", 0), ("specials", 0), ("fresh", 1), ("fresh_specials", 0), ("dst_only", 0)]
    out = []
    for j, (kind, pos) in enumerate(plan):
        rng = np.random.default_rng([77, j - (kind == "ties_swapped"), 0, 2])       # ties_swapped: the stream of ties, before it
        gen = {"fresh": "mixed", "fresh_specials": "specials", "dst_only": "specials", "ties_swapped": "ties"}.get(kind, kind)
        dst, src = make_pair_bgra(gen, rng, pos)
        if kind == "ties_swapped":
            dst, src = src, dst
        c = _case(_coord(j), kind, pos, dst.reshape(-1), src.reshape(-1))
        if kind.startswith("fresh"):
            c["dst"] = None
        elif kind == "dst_only":
            c["src"] = None
        else:
            c["pair"] = (dst, src)
        out.append(c)
    return out


BATCH_HELD = (0, 255, 510, 511, 512, 513, 514)


def batch_cases():
    """Gap 6: 515 pairs at 0 bands, 16S, over a 23 x 23 block of coordinates in a shuffled order (not the store's, which is by row).
    Returns (cases, images): case k's "src" is the index k % 4 into the four src images; dst holds the tiles at BATCH_HELD -- both
    ends of the first launch's table, the first entries of the second launch's and the entries around them -- each `mixed` against
    its own src image with a dst image of its own."""
    rng = np.random.default_rng([61, 0, 0, 0])
    block = [(x, y) for y in range(-11, 12) for x in range(-11, 12)]
    coords = [block[i] for i in rng.permutation(len(block))[:MERGE_BATCH + 3]]
    srcs = [make_pair("mixed", 0, 0, np.random.default_rng([61, 1 + q, 0, 0]), q)[1] for q in range(4)]
    images = [pack(*s, pad=SRC_PAD) for s in srcs]
    cases = []
    for k, t in enumerate(coords):
        dst = None
        if k in BATCH_HELD:
            d, _ = make_pair("mixed", 0, 0, np.random.default_rng([61, 10 + k, 0, 0]), k, src=srcs[k % 4])
            dst = pack(*d, pad=DST_PAD)
        cases.append(_case(t, "mixed" if dst is not None else "fresh", k, dst, k % 4))
    return cases, images


def state_cases(coords, bands=8, ff=1):
    """Gap 8: the records of a state file of more than one staging batch, one per coordinate (given in file order): `mixed` and
    `specials` src images in turn; dst holds the last two tiles of the first batch and the first two of the second, `mixed`.
    Returns (cases, records of the first batch)."""
    first = STAGE_BYTES // slot_layout(bands, ff)["total"]
    assert len(coords) == first + 3
    held = (first - 2, first - 1, first, first + 1)
    cases = []
    for k, t in enumerate(coords):
        kind = "mixed" if k % 2 == 0 or k in held else "specials"
        dst, src = make_pair(kind, bands, ff, np.random.default_rng([83, k, bands, int(bool(ff))]), k)
        cases.append(_case(t, kind, k, pack(*dst, pad=DST_PAD) if k in held else None, pack(*src, pad=SRC_PAD)))
    return cases, first


def zero_gaps(image, bands, ff):
    """a slot image as save_state writes it: the bytes that belong to no level are zeros"""
    return pack(*unpack(image, bands, ff), pad=0)


def expected(cases, images=None, bands=0, ff=0, single=False):
    """({t: bytes the map must hold after the merge}, won over the pairs whose dst was not fresh, pairs, fresh pairs)"""
    want, won, pairs, fresh = {}, 0, 0, 0
    for c in cases:
        src = c["src"] if images is None or c["src"] is None else images[c["src"]]
        if src is None:
            want[c["t"]] = np.asarray(c["dst"], np.uint8).reshape(-1)
            continue
        pairs += 1
        fresh += c["dst"] is None
        if single:
            img, w = merge_bgra(src if c["dst"] is None else c["dst"], src, c["dst"] is None)
        else:
            img, w = merge_slot(src if c["dst"] is None else c["dst"], src, bands, ff, c["dst"] is None)
        want[c["t"]] = img.reshape(-1)
        won += w
    return want, won, pairs, fresh


# ---------------------------------------------------------------- maps (these need the library)
def wide_poses(bands):
    """new_map's two prepare poses with the second moved far out: a grid of many tiles, for the state file's coordinates"""
    from test_gpu_model import lattice_poses
    p = lattice_poses(11 + bands)[:2]
    p[1][0] += 500.0; p[1][1] += 400.0
    return p


def new_single_band_map(pf):
    """the single-band counterpart of pyramid_inject.new_map: an empty prepared TypeCPU map"""
    from helpers import workloads
    from test_gpu_model import CAM, lattice_poses
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, lattice_poses(11)[:2])
    return g
