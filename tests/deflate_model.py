"""Test infrastructure for the lossless tile codec (include/pifusion.h, pf_deflate_tile_bgr): a plain Python encoder written from the
format's text -- predictor, run-length tokens, the length builder with its tie rules, the block plan, dynamic or stored, framing -- and the
hostile tiles the tests share.  zlib (the library) judges validity and supplies the Adler-32; this model judges the format.  Not part of
the product."""
import heapq
import zlib

import numpy as np

TILE = 256
ROW = 768
BLOCK = 16 * ROW
BLOCKS = 16
N = TILE * ROW
BOUND = N + 5 * BLOCKS + 6
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]      # RFC 1951 3.2.5
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def predict(tile):
    """256x256x3 BGR -> the N predicted bytes: RGB order, every sample minus the one before it in its row"""
    rgb = np.asarray(tile, np.uint8)[:, :, ::-1]
    p = rgb.copy()
    p[:, 1:] = rgb[:, 1:] - rgb[:, :-1]
    return np.ascontiguousarray(p).reshape(-1)


def unpredict(pred):
    """the N predicted bytes -> the 256x256x3 BGR tile"""
    rgb = np.cumsum(np.asarray(pred, np.uint8).reshape(TILE, TILE, 3).astype(np.uint32), axis=1).astype(np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def length_symbol(n):
    """match length -> (symbol, extra bits, their value); 258 has its own symbol"""
    if n == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= n)
    return 257 + i, LEN_EXTRA[i], n - LEN_BASE[i]


def tokens(block, prev):
    """block: the 12 288 bytes; prev: the byte before the block (None for block 0).  -> [(0, literal) | (1, match length)]"""
    b = np.asarray(block, np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(b[1:] != b[:-1]) + 1, [len(b)]))
    out = []
    for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        v = int(b[s])
        r = e - s
        if not (s == 0 and prev is not None and prev == v):
            out.append((0, v))
            r -= 1
        while r >= 258:
            out.append((1, 258))
            r -= 258
        if r >= 3:
            out.append((1, r))
        else:
            out += [(0, v)] * r
    return out


def code_lengths(freq, max_len):
    """the length builder of the format's text"""
    n = len(freq)
    assert 2 <= n <= 288 and 1 <= max_len <= 15 and (1 << max_len) >= n
    out = [0] * n
    used = sorted((int(f), i) for i, f in enumerate(freq) if f)          # by (count, index)
    if not used:
        return out
    if len(used) == 1:
        s = used[0][1]
        out[s] = 1
        out[1 if s == 0 else 0] = 1
        return out
    # Huffman: always the two lightest; of equal weights a leaf before an inner node, leaves in sorted order, inner nodes as made
    heap = [(f, 0, k, ("leaf", k)) for k, (f, _) in enumerate(used)]
    heapq.heapify(heap)
    made = 0
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], 1, made, ("node", a[3], b[3])))
        made += 1
    count = [0] * (max_len + 1)
    stack = [(heap[0][3], 0)]
    while stack:
        node, d = stack.pop()
        if node[0] == "leaf":
            count[min(d, max_len)] += 1
        else:
            stack.append((node[1], d + 1))
            stack.append((node[2], d + 1))
    total = sum(count[l] << (max_len - l) for l in range(1, max_len + 1))
    while total > (1 << max_len):
        count[max_len] -= 1
        for l in range(max_len - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    j = len(used)
    for l in range(1, max_len + 1):
        for _ in range(count[l]):
            j -= 1
            out[used[j][1]] = l
    return out


def canonical(lengths):
    """RFC 1951 3.2.2 -> [(code, length)], the code as a number whose most significant bit is sent first"""
    bl = [0] * 17
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + bl[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append((nxt[l], l))
        if l:
            nxt[l] += 1
    return out


def rle_lengths(seq):
    """the greedy run-length code of the code lengths -> [(symbol, extra bits, value)]"""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                c = min(r, 138)
                out.append((18, 7, c - 11))
                r -= c
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                c = min(r, 6)
                out.append((16, 2, c - 3))
                r -= c
            out += [(v, 0, 0)] * r
    return out


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    @property
    def at(self):
        return 8 * len(self.out) + self.n

    def put(self, v, n):          # low bit first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code_len):     # a Huffman code: its most significant bit first
        c, l = code_len
        self.put(int(format(c, "0%db" % l)[::-1], 2) if l else 0, l)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def plan(toks):
    """-> (literal/length lengths, header fields, bits of the dynamic block without its 3 first bits ... all of it)"""
    hist = [0] * 286
    for kind, v in toks:
        hist[v if kind == 0 else length_symbol(v)[0]] += 1
    hist[256] = 1
    ll = code_lengths(hist, 15)
    nlit = max(257, max(i for i in range(286) if ll[i]) + 1)
    rle = rle_lengths(ll[:nlit] + [1, 1])
    clfreq = [0] * 19
    for s, _, _ in rle:
        clfreq[s] += 1
    cl = code_lengths(clfreq, 7)
    ncl = 19
    while ncl > 4 and cl[CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    bits = 3 + 5 + 5 + 4 + 3 * ncl + sum(cl[s] + e for s, e, _ in rle)
    for kind, v in toks:
        if kind == 0:
            bits += ll[v]
        else:
            s, e, _ = length_symbol(v)
            bits += ll[s] + e + 1
    bits += ll[256]
    return ll, nlit, rle, cl, ncl, bits


def encode_pred(pred, info=None):
    """the stream of the N predicted bytes; info (a list) receives "dynamic" / "stored" per block"""
    pred = np.asarray(pred, np.uint8)
    assert pred.size == N
    w = Bits()
    w.put(0x78, 8)
    w.put(0x01, 8)
    for b in range(BLOCKS):
        blk = pred[b * BLOCK:(b + 1) * BLOCK]
        toks = tokens(blk, int(pred[b * BLOCK - 1]) if b else None)
        ll, nlit, rle, cl, ncl, bits = plan(toks)
        final = 1 if b == BLOCKS - 1 else 0
        stored = 3 + (-(w.at + 3)) % 8 + 32 + 8 * BLOCK
        if bits <= stored:
            if info is not None:
                info.append("dynamic")
            w.put(final, 1); w.put(2, 2)
            w.put(nlit - 257, 5); w.put(1, 5); w.put(ncl - 4, 4)
            for i in range(ncl):
                w.put(cl[CL_ORDER[i]], 3)
            clc = canonical(cl)
            for s, e, v in rle:
                w.huff(clc[s])
                w.put(v, e)
            llc = canonical(ll)
            rev = [int(format(c, "0%db" % l)[::-1], 2) if l else 0 for c, l in llc]
            for kind, v in toks:
                if kind == 0:
                    w.put(rev[v], ll[v])
                else:
                    s, e, x = length_symbol(v)
                    w.put(rev[s], ll[s]); w.put(x, e); w.put(0, 1)
            w.put(rev[256], ll[256])
        else:
            if info is not None:
                info.append("stored")
            w.put(final, 1); w.put(0, 2)
            w.align()
            w.put(BLOCK, 16); w.put(BLOCK ^ 0xFFFF, 16)
            assert w.n == 0
            w.out += blk.tobytes()
    w.align()
    return bytes(w.out) + zlib.adler32(pred.tobytes()).to_bytes(4, "big")


def encode_tile(tile, info=None):
    return encode_pred(predict(tile), info)


def zrle(pred):
    """the yardstick of size: zlib's own Z_RLE at level 6, window 15, of the same bytes"""
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(bytes(pred)) + c.flush()


# ---- the hostile tiles ---------------------------------------------------------------------------------------------------------------
def tile_of_pred(pred):
    return unpredict(pred)


def _noise(seed, n=N):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _runs_tile(seed, place):
    """noise without accidental runs, with runs of every hostile length of one value cut in at `place`"""
    rng = np.random.default_rng(seed)
    p = rng.integers(1, 17, N).astype(np.uint8)          # a small alphabet: the blocks come out dynamic
    same = np.flatnonzero(p[1:] == p[:-1]) + 1
    while same.size:                                     # no two equal neighbours in the filler
        p[same] = p[same] % 16 + 1
        same = np.flatnonzero(p[1:] == p[:-1]) + 1
    lens = [1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519]
    for k, r in enumerate(lens):
        b = 1 + k                                        # one block each: blocks 1 .. 12
        if place == "first":
            at = b * BLOCK
            p[at - 1] = 7                                # the byte before differs: no leaning
        elif place == "last":
            at = (b + 1) * BLOCK - r
        elif place == "across_lean":
            at = (b + 1) * BLOCK - r // 2 - 1            # the run goes on into the next block: that part leans
        elif place == "across_nolean":
            at = (b + 1) * BLOCK - r
            p[(b + 1) * BLOCK] = 0                        # ends with the block; the next block begins with another value
        else:                                            # "rowend": across the end of a row inside a block
            at = b * BLOCK + 5 * ROW - r // 2 - 1
        p[at:at + r] = 255 if place != "across_lean" else 254
        if at + r < N and place not in ("across_nolean",):
            if p[at + r] == p[at]:
                p[at + r] = 3
        if at > 0 and place != "first" and p[at - 1] == p[at]:
            p[at - 1] = 5
    # a run of a whole block, and one of a block that leans on the block before
    p[13 * BLOCK:14 * BLOCK] = 9
    p[13 * BLOCK - 1] = 8
    p[14 * BLOCK:15 * BLOCK] = 9 if place in ("across_lean", "first") else 10
    return p


def _fibonacci_block():
    """a block whose literal counts follow the Fibonacci numbers as far as 12 288 symbols go: the unlimited Huffman depth exceeds 15"""
    fib = [1, 2]                                         # with end-of-block, counted once: 1, 1, 2, 3, 5, ...
    while sum(fib) + fib[-1] + fib[-2] <= BLOCK - 1:
        fib.append(fib[-1] + fib[-2])
    groups = sorted([(c, v) for v, c in enumerate(fib)], reverse=True)      # the most frequent value first
    rest = BLOCK - sum(fib)
    groups = sorted(groups + [(rest, 200)], reverse=True)                   # what remains: one other value
    vals = [v for c, v in groups for _ in range(c)]
    a = np.zeros(BLOCK, np.uint8)
    a[0::2] = vals[:BLOCK // 2]                          # even places, then odd ones: no value meets itself (none fills half the block)
    a[1::2] = vals[BLOCK // 2:]
    assert not (a[1:] == a[:-1]).any()
    return a


def hostile_preds():
    """{name: the N predicted bytes}"""
    out = {}
    out["zeros"] = np.zeros(N, np.uint8)
    out["last_differs"] = np.zeros(N, np.uint8); out["last_differs"][-1] = 1
    out["noise"] = _noise(1)
    for place in ("first", "last", "across_lean", "across_nolean", "rowend"):
        out["runs_" + place] = _runs_tile(11, place)
    one = _noise(2)
    one[3 * BLOCK:4 * BLOCK] = np.where(np.arange(BLOCK) % 600 == 0, 77, 0)      # zeros in long runs and one literal value besides
    one[3 * BLOCK] = 0
    one[4 * BLOCK - 1] = 0
    out["two_symbols"] = one
    single = np.zeros(N, np.uint8)
    single[5 * BLOCK:6 * BLOCK] = 42                                             # a block of ONE literal value: literal, matches, end-of-block
    out["one_literal"] = single
    fibt = _noise(3)
    fibt[2 * BLOCK:3 * BLOCK] = _fibonacci_block()
    out["fibonacci"] = fibt
    smooth = (np.cumsum(np.random.default_rng(4).integers(-2, 3, N)) // 4).astype(np.uint8)
    out["smooth"] = smooth
    return out


def hostile_tiles():
    """{name: 256x256x3 BGR}; "all255" is given as pixels (its predicted bytes are 255 then zeros)"""
    t = {k: tile_of_pred(v) for k, v in hostile_preds().items()}
    t["all255"] = np.full((TILE, TILE, 3), 255, np.uint8)
    return t
