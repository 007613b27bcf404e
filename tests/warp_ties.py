"""Homographies that put the level-0 warp's fp64 coordinates ON the rounding boundaries of cvRound, and a mutation harness that shows
they do -- test code only.

warpPerspective's coordinate (OpenCV 2.4.9 imgwarp.cpp, SURVEY 8c rule 2) is cvRound((X0 + M0*x1) * (32 / W)): about 2^15 with an ulp of
2^-37, so with the homography of a jittered pose a 1-ulp error anywhere in the chain moves a 1/32-px coordinate on one pixel in ~2^37, and
no parity test sees it.  The matrices below have small dyadic entries, W a small integer or a power of two on whole rows, so that
thousands of pixels per canvas are exact `.5` ties (or, for the ulp-nudged copies, within a few ulps of one) at scale 32, at scale 1
(the weight's nearest coordinate), or both -- among them the ties that decide the frame's border: p = -1/2, p = cols - 1/2 at scale 1,
p = -1/64, p = cols - 1 - 1/64 and the last two rows (warp_index.hpp tap_is_fast) at scale 32.

MATRICES: (name, M0), M0 = frame -> canvas, the direction perspective_transform returns and the oracle's ops take; each is
map_model.invert3x3(A) of the wanted canvas -> source matrix A, and what the kernels, the oracle and the model then work with is
invert3x3(M0): whatever cv::invert's closed form made of A (for the `exact_*` family: A itself, bit for bit).

MUTANTS / mutant_coords(): a plain restatement of map_model._warp_coords with one link of the chain changed at a time; flipped() counts
the canvas pixels whose rounded coordinates change.  tests/test_warp_ties.py asserts that every mutant is seen on MATRICES and none
(but the fp32 one) on the generic CONTROL; tests/test_gpu_warp_ties.py feeds the same matrices to the HIP kernels."""
import numpy as np

from map_model import invert3x3

CANVAS = (512, 768)             # rows, cols of the CPU qualification: 2 x 3 tiles
FRAME = (480, 640)              # rows, cols of the frames the matrices are made for
LD = np.longdouble

# ---------------------------------------------------------------- the matrices
_D = [[105 / 64, 3 / 128, 7.5], [-5 / 256, 105 / 64, 3.25]]                    # rows 0 / 1 of the dyadic affine map
_BASE = [
    # every odd x is an exact tie of 32 * X (105/64 * 32 = 52.5)
    ("aff_dyadic", [_D[0], _D[1], [0, 0, 1]]),
    # the same map with W = 3: the rounding of 32/3 decides every one of those ties
    ("aff_dyadic_w3", [[3 * v for v in _D[0]], [3 * v for v in _D[1]], [0, 0, 3]]),
    # W = 1 + y/256; and with M6 = 1/1024 as well: ties on the rows and columns where W divides the numerators
    ("proj_y", [_D[0], _D[1], [0, 1 / 256, 1]]),
    ("proj_xy", [_D[0], _D[1], [1 / 1024, 1 / 256, 1]]),
    # W = 5 on the first row, growing along y: a reciprocal that is not a power of two times a dyadic numerator
    ("proj_w5", [[5 * v for v in _D[0]], [5 * v for v in _D[1]], [0, 5 / 512, 5]]),
]
# closed-form inverse exact in both directions (unimodular shears; scales 2 and 1/2): exact ties in the arithmetic the kernels see.
# The offsets put the ties on the frame's border decisions (frame = FRAME, canvas = CANVAS or larger):
_EXACT = [
    # scale 32: 32 Y = 32 y - 672.5 ties on every pixel, 32 X on every even row; X = -1/64 at (37, 0), X = 639 - 1/64 at (676, 0),
    # Y = -1/64 on canvas row 21, Y = 478 - 1/64 and 479 - 1/64 on rows 499 and 500 (the two rows tap_is_fast excludes)
    ("exact_shear_32", [[1, 1 / 64, -37 - 1 / 64], [0, 1, -21 - 1 / 64], [0, 0, 1]]),
    # scale 1: Y = y - 21.5 ties on every pixel (-1/2 on row 21: in bounds only under half-even; 479.5 on row 501), X on every 64th row
    # (-1/2 at (37, 0), 639.5 at (677, 0))
    ("exact_shear_1", [[1, 1 / 64, -37.5], [0, 1, -21.5], [0, 0, 1]]),
    # scale 2: X = 2 x - 60.5 ties at scale 1 on every pixel (-1/2 at x = 30, 639.5 at x = 350), 32 Y = 64 y - 1280.5 at scale 32
    ("exact_scale_2", [[2, 0, -60.5], [0, 2, -40 - 1 / 64], [0, 0, 1]]),
    # scale 1/2: 32 X = 16 x - 640.5 ties on every pixel, Y = y/2 - 10 at scale 1 on every odd row (-1/2 on row 19)
    ("exact_scale_half", [[0.5, 0, -20 - 1 / 64], [0, 0.5, -10], [0, 0, 1]]),
]
# a matrix of the kind every other test produces (a jittered pose): the control
_CONTROL = ("control", [[1.6180339887498949, 0.023344556677889901, 7.1234567890123457],
                        [-0.019988776655443322, 1.6398765432109876, 3.2345678901234567],
                        [1.2345678901234568e-05, -2.3456789012345679e-05, 1.0]])


def _nudged(A, seed):
    """every non-zero entry of A moved by 0 ... +-3 ulps: exact ties become near-ties, which operation order and contraction can flip"""
    rng = np.random.RandomState(seed)
    out = np.array(A, np.float64)
    for i in range(3):
        for j in range(3):
            k = int(rng.randint(-3, 4))
            for _ in range(abs(k)):
                if out[i, j] != 0.0:
                    out[i, j] = np.nextafter(out[i, j], np.inf if k > 0 else -np.inf)
    return out


def _build():
    src = list(_BASE) + list(_EXACT)
    for s, (name, A) in enumerate(_BASE + _EXACT[:2]):
        src.append((name + "_ulp", _nudged(A, 100 + s)))
    for s, (name, A) in enumerate(_BASE[:4]):
        src.append((name + "_ulp2", _nudged(A, 200 + s)))
    src.append(_CONTROL)
    return [(name, invert3x3(np.array(A, np.float64))) for name, A in src]


MATRICES = _build()
NAMES = [n for n, _ in MATRICES]
CONTROL = "control"
EXACT = [n for n, _ in _EXACT]


def matrix(name):
    return MATRICES[NAMES.index(name)][1]


def wanted(name):
    """the canvas -> source matrix A an `exact_*` entry was built from"""
    return np.array(dict(_EXACT)[name], np.float64)


# ---------------------------------------------------------------- the mutation harness
MUTANTS = ("rcp_up", "rcp_dn", "div", "half_away", "half_up", "fma_row", "fma_col", "order", "noblock", "w_f32")


def fma(a, b, c):
    """RN(a * b + c) of doubles a, c and small integers b (|b| < 2^11), in numpy.longdouble: the product has at most 64 significant
    bits and is exact there; the sum is rounded to 64 bits and then to 53, and where the first rounding was inexact and landed on the
    middle between two doubles the second one is taken towards the side the lost part (TwoSum) lies on."""
    assert np.finfo(LD).nmant >= 63, "needs an extended-precision long double"
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    assert np.abs(b).max() < 2048 and (b == np.rint(b)).all()
    p = a.astype(LD) * b.astype(LD)
    cl = c.astype(LD)
    s = cl + p
    t = s - cl
    err = (cl - (s - t)) + (p - t)                     # TwoSum: s + err == c + a * b exactly
    d = s.astype(np.float64)
    r = s - d.astype(LD)                                # exact
    tie = (np.abs(r) == (np.spacing(np.abs(d)) / 2).astype(LD)) & (err != 0)
    other = (d.astype(LD) + 2 * r).astype(np.float64)   # the double on the other side of s
    return np.where(tie & (np.sign(err) == np.sign(r)), other, d)


def _round(v, how):
    v = np.clip(v, -2.0 ** 31, 2.0 ** 31 - 1)
    if how == "even":
        return np.rint(v).astype(np.int64)
    lo = np.floor(v)
    up = (v - lo) >= 0.5                                # v - floor(v) is exact
    if how == "away":                                   # half away from zero: a negative tie goes down
        up = np.where(v < 0, (v - lo) > 0.5, up)
    return (lo + up).astype(np.int64)


def mutant_coords(M, drows, dcols, scales, mutant=None):
    """map_model._warp_coords restated (per scale: cvRound of both coordinates), with one link changed:
      rcp_up / rcp_dn   scale / W one ulp up / down
      div               (numerator * scale) / W instead of numerator * (scale / W)
      half_away/half_up cvRound's tie rule
      fma_row           the row terms M0*xb + M1*y + M2 with the second product contracted into the sum
      fma_col           W0 + M6*x1, X0 + M0*x1, Y0 + M3*x1 contracted
      order             the row terms summed as M0*xb + (M1*y + M2)
      noblock           M0*x + M1*y + M2 from the pixel's x instead of from its 64-wide block origin
      w_f32             W rounded through fp32"""
    M = np.asarray(M, np.float64).reshape(3, 3)
    bw0 = min(1024 // min(16, drows), dcols)
    x = np.arange(dcols)
    xb = (x // bw0) * bw0; x1 = x - xb
    if mutant == "noblock":
        xb, x1 = x, np.zeros_like(x)
    yf, xbf, x1f = np.arange(drows, dtype=np.float64)[:, None], xb.astype(np.float64)[None, :], x1.astype(np.float64)[None, :]

    def row(r):
        if mutant == "fma_row":
            return fma(M[r, 1], yf, M[r, 0] * xbf) + M[r, 2]
        if mutant == "order":
            return M[r, 0] * xbf + (M[r, 1] * yf + M[r, 2])
        return M[r, 0] * xbf + M[r, 1] * yf + M[r, 2]

    def col(r, base):
        if mutant == "fma_col":
            return fma(M[r, 0], x1f, base)
        return base + M[r, 0] * x1f

    W = col(2, row(2)); nX = col(0, row(0)); nY = col(1, row(1))
    if mutant == "w_f32":
        W = W.astype(np.float32).astype(np.float64)
    nz = W != 0
    Wd = np.where(nz, W, 1)
    how = {"half_away": "away", "half_up": "up"}.get(mutant, "even")
    out = []
    for scale in scales:
        Ws = np.where(nz, scale / Wd, 0.0)
        if mutant == "rcp_up":
            Ws = np.nextafter(Ws, np.inf)
        elif mutant == "rcp_dn":
            Ws = np.nextafter(Ws, -np.inf)
        if mutant == "div":
            fX = np.where(nz, (nX * scale) / Wd, 0.0); fY = np.where(nz, (nY * scale) / Wd, 0.0)
        else:
            fX, fY = nX * Ws, nY * Ws
        out.append((_round(fX, how), _round(fY, how)))
    return out


def flipped(base, mut):
    """per scale: canvas pixels whose rounded coordinate pair differs between two results of mutant_coords"""
    return [int(((X != X0) | (Y != Y0)).sum()) for (X0, Y0), (X, Y) in zip(base, mut)]


# ---------------------------------------------------------------- a model's tiles on their way to another process
class StoredMap:
    """The tiles of a ModelMap / ModelMapSingleBand, written to and read from one .npz: what helpers.compare_with_model and
    compare_single_with_model read of a model."""

    def __init__(self, path):
        z = np.load(path)
        self.num_levels = int(z["num_levels"])
        self._tiles = [tuple(int(v) for v in t) for t in z["tiles"]]
        self._z = {k: z[k] for k in z.files}

    @staticmethod
    def save(path, m):
        out = {"num_levels": np.int64(m.num_levels), "tiles": np.array(m.tiles(), np.int64).reshape(-1, 2)}
        for (ix, iy) in m.tiles():
            if hasattr(m, "tile_bgra"):
                out["b_%d_%d" % (ix, iy)] = m.tile_bgra(ix, iy)
            else:
                for lv in range(m.num_levels):
                    out["l_%d_%d_%d" % (ix, iy, lv)], out["w_%d_%d_%d" % (ix, iy, lv)] = m.tile_level(ix, iy, lv)
        np.savez(path, **out)

    def tiles(self):
        return list(self._tiles)

    def tile_level(self, ix, iy, lv):
        return self._z["l_%d_%d_%d" % (ix, iy, lv)], self._z["w_%d_%d_%d" % (ix, iy, lv)]

    def tile_bgra(self, ix, iy):
        return self._z["b_%d_%d" % (ix, iy)]


# ---------------------------------------------------------------- the GPU side (tests/test_gpu_warp_ties.py)
CAM = [640, 480, 500, 500, 320, 240]
# two canvases of 3 x 3 tiles, one tile apart: the keyframes compete where they overlap, and every frame border is stored somewhere
POSES = [[0.0, 0.0, -100.0, 0, 0, 0, 1], [51.2, 0.0, -100.0, 0, 0, 0, 1]]
# (matrix, pose): exact ties at scale 32 and on the tap borders; exact ties at scale 1 and on the weight's borders; near-ties behind a
# reciprocal that is not a power of two (division, column terms, block origin); near-ties of a shear (operation order, column terms);
# the W = 3 map nudged otherwise (row terms); a projective W = 5 (1 + y / 512) -- and that one again, so that every weight ties and the
# newest keyframe must win.  With the int16 model's coordinates replaced by each mutant's in turn, the level-0 pixels STORED after these
# seven feeds differ on (Laplacian / weight): rcp_up 159 371 / 2 526, rcp_dn 261 029 / 3 447, div 9 118 / 58, half_away 140 503 / 2 259,
# half_up 140 389 / 2 255, fma_row 104 / 1, fma_col 12 407 / 37, order 8 300 / 0, noblock 23 691 / 77, w_f32 154 762 / 1 586.
FEEDS = [("exact_shear_32", 0), ("exact_scale_2", 0), ("aff_dyadic_w3_ulp2", 0), ("exact_shear_32_ulp", 1), ("aff_dyadic_w3_ulp", 1),
         ("proj_w5", 1), ("proj_w5", 1)]


def feed_frame(k):
    from helpers import workloads
    return workloads().noise_frame(FRAME[0], FRAME[1], 300 + k)


def run_cases(spec):
    """The child process of tests/test_gpu_warp_ties.py: the library PF_LIB names (the experiments build: the hook exists there alone),
    under the switches of this process' environment.  spec: {"models": {pyramid type: .npz of the model's map}, "cases": [{"id", "type":
    "i16" | "f32" | "single", "options": pf_options fields, "cull": bool, "inject": bool, "bgra": bool}]}; with "bgra" the keyframes are fed
    as BGRA, bgra.with_alpha(feed_frame(k), k): the colour content, and so the models, are the same.  Returns {"forms":
    pf_debug_form_counts, "seconds": what the cases took, case id: mismatch strings against the model}."""
    import ctypes as C
    import time
    import bgra
    from conftest import load_package
    from helpers import compare_with_model, workloads
    pf = load_package(); wl = workloads()
    out = {}
    four = {}                                           # the BGRA keyframes, made once
    t0 = time.perf_counter()
    for c in spec["cases"]:
        opt = dict(c.get("options", {}))
        if c["type"] == "single":
            g = pf.Map2D.create(pf.TypeCPU, False, **opt)
        else:
            g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=int(c["type"] == "f32"), **opt)
        if "cull" in c:
            g.set_cull(bool(c["cull"]))
        assert g.prepare(wl.IDENTITY_PLANE, CAM, POSES)
        for k, (name, p) in enumerate(FEEDS):
            if c.get("inject", True):
                g.next_homography(matrix(name))
            if c.get("bgra") and k not in four:
                four[k] = bgra.with_alpha(feed_frame(k), k)
            assert g.feed(four[k] if c.get("bgra") else feed_frame(k), POSES[p])
        assert g.sync()
        m = StoredMap(spec["models"][c["type"]])
        if c["type"] == "single":
            bad = ["tile sets differ"] if g.tiles() != m.tiles() else []
            for t in (m.tiles() if not bad else []):
                d = g.tile_bgra(*t) != m.tile_bgra(*t)
                if d.any():
                    bad.append("tile_bgra %s: %d px differ (%d in alpha)" % (t, int(d.any(axis=2).sum()), int(d[:, :, 3].sum())))
        else:
            bad = compare_with_model(g, m, blends=False)
        out[c["id"]] = bad
        g.close()
    cnt = (C.c_longlong * 8)(); pf.lib().pf_debug_form_counts(cnt)
    out["forms"] = list(cnt)
    out["seconds"] = time.perf_counter() - t0
    return out
