"""Independent numpy models of MultiBandMap2DCPU (Map2DFusion/MultiBandMap2DCPU.cpp) and, at the end, of Map2DCPU, test code only.

Written from SURVEY 3.2/3.3 and 8c rules 2-9 and from reading the reference's renderFrame (.cpp:311-558), Ele::blend (.cpp:77-146)
and save (.cpp:779-847).  It shares no pixel arithmetic with the oracle (oracle/oracle.c) or the HIP library: the geometry a feed
needs -- the grid after the feed, the footprint in plane coordinates and the homography M -- comes in from outside (the homography
solver is the documented deviation, SURVEY 8c rule 1), everything after it is computed here.

int16 maps are modelled in exact int64 arithmetic with the casts and saturations of the rules; fp32 maps in float32 with the
operation order of the rules (numpy rounds every float32 operation, and never contracts a multiply-add).
"""
import math

import numpy as np

ELE = 256
F = np.float32


# ---------------------------------------------------------------- op-level restatements (also pinned by test_oracle_ops.py)
def np_pyr_down_int(src):
    """5x5 [1 4 6 4 1]^2, REFLECT_101, ((v+128)>>8) -- exact integer arithmetic."""
    s = src.astype(np.int64)
    p = np.pad(s, ((2, 2), (2, 2), (0, 0)), mode="reflect")
    k = np.array([1, 4, 6, 4, 1], np.int64)
    h = sum(k[j] * p[:, j:j + s.shape[1]:1] for j in range(5))[:, ::2]
    h = h[:, :(s.shape[1] + 1) // 2]
    v = sum(k[j] * h[j:j + s.shape[0]] for j in range(5))[::2][:(s.shape[0] + 1) // 2]
    return ((v + 128) >> 8).astype(np.int16)


def np_pyr_up_int(src):
    """pyrUp to 2x: even = p[x-1]+6p[x]+p[x+1], odd = 4(p[x]+p[x+1]); index -1 -> 1, n -> n-1."""
    s = src.astype(np.int64)

    def up_axis(a, axis):
        a = np.moveaxis(a, axis, 0)
        n = a.shape[0]
        prev = a[[1 if n > 1 else 0] + list(range(0, n - 1))]
        nxt = a[list(range(1, n)) + [n - 1]]
        out = np.empty((2 * n,) + a.shape[1:], np.int64)
        out[0::2] = prev + 6 * a + nxt
        out[1::2] = 4 * (a + nxt)
        return np.moveaxis(out, 0, axis)

    v = up_axis(up_axis(s, 1), 0)
    return ((v + 32) >> 6).astype(np.int16)


def np_warp_linear_reflect(src, M0, drows, dcols, as_float):
    """warpPerspective LINEAR/REFLECT with the 64-wide block-relative coordinates, vectorised."""
    M = np.linalg.inv(np.asarray(M0, np.float64))      # only used with exactly invertible test matrices
    return warp_linear_reflect_inv(src, M, drows, dcols, as_float)


# ---------------------------------------------------------------- geometry shared by both warps
def invert3x3(S):
    """cv::invert's closed form for 3x3 doubles (core/src/lapack.cpp, n == 3): cofactors times 1/det; singular -> zeros."""
    s = [[float(v) for v in r] for r in np.asarray(S, np.float64).reshape(3, 3)]
    d = (s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1])
         - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0])
         + s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]))
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    return np.array([[(s[1][1] * s[2][2] - s[1][2] * s[2][1]) * d, (s[0][2] * s[2][1] - s[0][1] * s[2][2]) * d,
                      (s[0][1] * s[1][2] - s[0][2] * s[1][1]) * d],
                     [(s[1][2] * s[2][0] - s[1][0] * s[2][2]) * d, (s[0][0] * s[2][2] - s[0][2] * s[2][0]) * d,
                      (s[0][2] * s[1][0] - s[0][0] * s[1][2]) * d],
                     [(s[1][0] * s[2][1] - s[1][1] * s[2][0]) * d, (s[0][1] * s[2][0] - s[0][0] * s[2][1]) * d,
                      (s[0][0] * s[1][1] - s[0][1] * s[1][0]) * d]])


def _warp_coords(M, drows, dcols, scales):
    """warpPerspectiveInvoker: the destination in blocks of bw0 = min(1024 / min(16, rows), cols) columns, each pixel's source
    coordinate evaluated from its block's x origin in double; scale 32 (INTER_LINEAR: 1/32-px grid) or 1 (INTER_NEAREST).
    Returns, per scale, cvRound of both coordinates, clamped to int first."""
    y, x = np.mgrid[0:drows, 0:dcols]
    bw0 = min(1024 // min(16, drows), dcols)
    xb = (x // bw0) * bw0; x1 = x - xb
    X0 = M[0, 0] * xb + M[0, 1] * y + M[0, 2]
    Y0 = M[1, 0] * xb + M[1, 1] * y + M[1, 2]
    W0 = M[2, 0] * xb + M[2, 1] * y + M[2, 2]
    W = W0 + M[2, 0] * x1
    nX, nY = X0 + M[0, 0] * x1, Y0 + M[1, 0] * x1
    out = []
    for scale in scales:
        Ws = np.where(W != 0, scale / np.where(W != 0, W, 1), 0.0)
        out.append((np.rint(np.clip(nX * Ws, -2 ** 31, 2 ** 31 - 1)).astype(np.int64),
                    np.rint(np.clip(nY * Ws, -2 ** 31, 2 ** 31 - 1)).astype(np.int64)))
    return out


def warp_linear_reflect_inv(src, M, drows, dcols, as_float, XY=None):
    """INTER_LINEAR + BORDER_REFLECT with the inverse map M given: float taps ((1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx), summed
    left to right in float; 16S output = saturate(cvRound(sum)).  XY: the scale-32 coordinates when already computed."""
    srows, scols, cn = src.shape
    X, Y = XY if XY is not None else _warp_coords(M, drows, dcols, (32.0,))[0]
    sx = np.clip(X >> 5, -32768, 32767); sy = np.clip(Y >> 5, -32768, 32767)
    fx = ((X & 31).astype(np.float32) * np.float32(1 / 32)); fy = ((Y & 31).astype(np.float32) * np.float32(1 / 32))

    def refl(p, n):
        p = np.mod(p, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)

    x0, x1_, y0, y1 = refl(sx, scols), refl(sx + 1, scols), refl(sy, srows), refl(sy + 1, srows)
    one = np.float32(1)
    w = [(one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx]
    s = src.astype(np.float32).reshape(-1, cn)
    t = s[y0 * scols + x0] * w[0][..., None]
    t = t + s[y0 * scols + x1_] * w[1][..., None]
    t = t + s[y1 * scols + x0] * w[2][..., None]
    t = t + s[y1 * scols + x1_] * w[3][..., None]
    if as_float:
        return t
    return np.clip(np.rint(t.astype(np.float64)), -32768, 32767).astype(np.int16)


def warp_nearest_const_inv(src, M, drows, dcols, XY=None):
    """INTER_NEAREST + BORDER_CONSTANT(0) of a 1-channel float image (the weight warp, .cpp:454).  XY: the scale-1 coordinates."""
    srows, scols = src.shape
    X, Y = XY if XY is not None else _warp_coords(M, drows, dcols, (1.0,))[0]
    sx = np.clip(X, -32768, 32767); sy = np.clip(Y, -32768, 32767)
    inside = (sx >= 0) & (sx < scols) & (sy >= 0) & (sy < srows)
    return np.where(inside, src[np.clip(sy, 0, srows - 1), np.clip(sx, 0, scols - 1)], np.float32(0)).astype(np.float32)


def weight_image(rows, cols, weight_type):
    """.cpp:400-418, all in float; w/2 and h/2 are integer divisions."""
    xc, yc = F(cols // 2), F(rows // 2)
    dmax = np.sqrt(xc * xc + yc * yc, dtype=np.float32)
    i, j = np.mgrid[0:rows, 0:cols].astype(np.float32)
    d = (i - yc) * (i - yc) + (j - xc) * (j - xc)
    e = F(1) - np.sqrt(d, dtype=np.float32) / dmax
    if weight_type:
        e = e * e
    return np.where(e.astype(np.float64) <= 1e-5, F(1e-5), e).astype(np.float32)


# ---------------------------------------------------------------- pyramids (SURVEY 8c rules 4-8)
def _reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.mod(p, 2 * n - 2)
    return np.where(p < n, p, 2 * n - 2 - p)


def pyr_down(a, stats=None):
    """cv::pyrDown of an (rows, cols, cn) int16 or float32 image.  int16: exact int64 sums, (v + 128) >> 8.  float32: horizontal
    s2*6 + (s1+s3)*4 + s0 + s4; vertical in the SSE order ((r0+r4)+(r2+r2)) + ((r1+r3)+r2)*4 on the first floor(w*cn/8)*8 floats
    of a row and in the scalar order r2*6 + (r1+r3)*4 + r0 + r4 on the rest, then * (1/256).  stats (int16 only) records the
    largest horizontal and vertical sums."""
    rows, cols, cn = a.shape
    is_f = a.dtype == np.float32
    s = a if is_f else a.astype(np.int64)
    c6, c4 = (F(6), F(4)) if is_f else (6, 4)
    xs = 2 * np.arange((cols + 1) // 2)
    i0, i1, i2, i3, i4 = (_reflect101(xs + d, cols) for d in (-2, -1, 0, 1, 2))
    h = s[:, i2] * c6 + (s[:, i1] + s[:, i3]) * c4 + s[:, i0] + s[:, i4]
    ys = 2 * np.arange((rows + 1) // 2)
    r0, r1, r2, r3, r4 = (h[_reflect101(ys + d, rows)] for d in (-2, -1, 0, 1, 2))
    if not is_f:
        v = r2 * 6 + (r1 + r3) * 4 + r0 + r4
        if stats is not None:
            stats["h5"] = max(stats.get("h5", 0), int(np.abs(h).max()))
            stats["v5"] = max(stats.get("v5", 0), int(np.abs(v).max()))
        return ((v + 128) >> 8).astype(np.int16)          # FixPtCast<int, short, 8>: no saturation
    sca = (r2 * c6 + (r1 + r3) * c4 + r0 + r4) * F(1 / 256)
    vec = (((r0 + r4) + (r2 + r2)) + ((r1 + r3) + r2) * c4) * F(1 / 256)
    dw = h.shape[1] * cn
    j = (np.arange(h.shape[1])[:, None] * cn + np.arange(cn)[None, :])          # float index within the row
    return np.where((j < (dw // 8) * 8)[None], vec, sca).astype(np.float32)


def pyr_up(a, stats=None):
    """cv::pyrUp to exactly twice the size.  Columns: x=0 -> s0*6 + s1*2 and (s0+s1)*4; inner x -> s[x-1] + s[x]*6 + s[x+1] and
    (s[x]+s[x+1])*4; x=n-1 -> s[n-2] + s[n-1]*7 and s[n-1]*8; a single column -> s*8 twice.  Rows: r0 + r1*6 + r2 and (r1+r2)*4,
    row -1 reflected to row 1, row n replicated to row n-1.  int16: (v + 32) >> 6 without saturation; float32: v * (1/64)."""
    rows, cols, cn = a.shape
    is_f = a.dtype == np.float32
    s = a if is_f else a.astype(np.int64)
    c2, c4, c6, c7, c8 = (F(2), F(4), F(6), F(7), F(8)) if is_f else (2, 4, 6, 7, 8)
    h = np.empty((rows, 2 * cols, cn), s.dtype)
    if cols == 1:
        h[:, 0] = s[:, 0] * c8; h[:, 1] = s[:, 0] * c8
    else:
        h[:, 0] = s[:, 0] * c6 + s[:, 1] * c2
        h[:, 1] = (s[:, 0] + s[:, 1]) * c4
        h[:, 2:-2:2] = s[:, :-2] + s[:, 1:-1] * c6 + s[:, 2:]
        h[:, 3:-2:2] = (s[:, 1:-1] + s[:, 2:]) * c4
        h[:, -2] = s[:, -2] + s[:, -1] * c7
        h[:, -1] = s[:, -1] * c8
    y = np.arange(rows)
    r0 = h[np.where(y - 1 < 0, min(1, rows - 1), y - 1)]
    r1 = h
    r2 = h[np.minimum(y + 1, rows - 1)]
    out = np.empty((2 * rows, 2 * cols, cn), s.dtype)
    out[0::2] = r0 + r1 * c6 + r2
    out[1::2] = (r1 + r2) * c4
    if is_f:
        return (out * F(1 / 64)).astype(np.float32)
    if stats is not None:
        stats["up"] = max(stats.get("up", 0), int(np.abs(out).max()))
    return ((out + 32) >> 6).astype(np.int16)             # FixPtCast<int, short, 6>: no saturation


def _sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def create_laplace_pyr(img, n, stats=None):
    """blenders.cpp createLaplacePyr (non-8U): Gaussian levels first, then L_i = G_i - pyrUp(G_{i+1}), saturating for 16S."""
    g = [img]
    for _ in range(n):
        g.append(pyr_down(g[-1], stats))
    out = []
    for i in range(n):
        up = pyr_up(g[i + 1], stats)
        if img.dtype == np.float32:
            out.append(g[i] - up)
        else:
            out.append(_sat16(g[i].astype(np.int64) - up.astype(np.int64)))
    out.append(g[n])
    if stats is not None and img.dtype == np.int16 and n:
        stats["lap"] = max(stats.get("lap", 0), max(int(np.abs(l.astype(np.int64)).max()) for l in out[:n]))
    return out


def restore_from_laplace_pyr(levels):
    """blenders.cpp restoreImageFromLaplacePyr: from the top, G_{i-1} = pyrUp(G_i) + L_{i-1} (saturating add for 16S)."""
    lv = list(levels)
    for i in range(len(lv) - 1, 0, -1):
        up = pyr_up(lv[i])
        if up.dtype == np.float32:
            lv[i - 1] = up + lv[i - 1]
        else:
            lv[i - 1] = _sat16(up.astype(np.int64) + lv[i - 1].astype(np.int64))
    return lv[0]


def to_8u(raw):
    """8U view: 16S saturated; fp32 by the project's rule saturate(cvRound(v * 255.f)) (oracle.c's updateTexture / save views)."""
    if raw.dtype == np.int16:
        return np.clip(raw.astype(np.int64), 0, 255).astype(np.uint8)
    return np.clip(np.rint((raw * F(255)).astype(np.float64)), 0, 255).astype(np.uint8)


def canvas_geometry(shape, grid, footprint, M, check_M=True):
    """renderFrame's tile range and canvas points (MultiBandMap2DCPU.cpp:380-391, :437-438; Map2DCPU.cpp:219-233, :290-296 are the same
    lines) from the grid after the feed, the footprint in plane coordinates and M, which must map the frame onto those points.
    check_M=False: M is a matrix a test chose (tests/warp_ties.py) and is taken as it is.
    Returns ((off_x, off_y), (x0, y0, x1, y1) as dense tile indices, canvas points as float32, M as 3 x 3 float64)."""
    (w, h, offx, offy), (mnx, mny, _, _, ele_size, length_pixel) = grid
    pts = np.asarray(footprint, np.float64).reshape(4, 2)
    xmin, ymin = pts[:, 0].min(), pts[:, 1].min()
    xmax, ymax = pts[:, 0].max(), pts[:, 1].max()
    inv = 1.0 / ele_size                                                        # eleSizeInv
    x0 = int(math.floor((xmin - mnx) * inv)); y0 = int(math.floor((ymin - mny) * inv))      # .cpp:380-383
    x1 = int(math.ceil((xmax - mnx) * inv)); y1 = int(math.ceil((ymax - mny) * inv))
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h, "footprint outside the grid it was given"
    cx, cy = mnx + ele_size * x0, mny + ele_size * y0                           # .cpp:390-391
    lpi = 1.0 / length_pixel
    canvas = np.array([[(p[0] - cx) * lpi, (p[1] - cy) * lpi] for p in pts], np.float32)   # Point2f, .cpp:437-438
    M = np.asarray(M, np.float64).reshape(3, 3)
    rows, cols = shape[:2]
    corners = np.array([[0, 0], [cols, 0], [0, rows], [cols, rows]], np.float64)
    proj = (M @ np.c_[corners, np.ones(4)].T).T
    assert not check_M or np.abs(proj[:, :2] / proj[:, 2:] - canvas).max() < 1e-3, "M does not map the frame onto its canvas points"
    return (offx, offy), (x0, y0, x1, y1), canvas, M


# ---------------------------------------------------------------- the map
class ModelMap:
    """MultiBandMap2DCPU, thread=false, one renderFrame per feed.  Tiles are keyed by world tile (ix, iy) = dense index + grid
    offset, so the state follows the origin when spreadMap moves it."""

    def __init__(self, band_num=5, force_float=0, weight_type=0, high_quality=1, bg_color=0):
        self.L = min(band_num, int(math.ceil(math.log(ELE) / math.log(2.0))))       # .cpp:260-263
        self.force_float = force_float
        self.dtype = np.float32 if force_float else np.int16
        self.weight_type = weight_type
        self.high_quality = high_quality
        self.bg_color = bg_color
        self.tiles_ = {}                    # (ix, iy) -> ([lap_0 .. lap_L], [w_0 .. w_L])
        self.grid_ = None
        self.stats = {}                     # int16: largest |sums| of the level pyramid (h5, v5, up) and |Laplacian| (lap)
        self.last = None                    # ([x0, y0, tx, ty], canvas points as float32, M) of the last feed
        self._wimg = None
        self._out = {}                      # blends and the save of the current state, each computed once

    @property
    def num_levels(self):
        return self.L + 1

    def feed(self, bgr, grid, footprint, M, check_M=True):
        """One keyframe.  grid: (dims, geo) of the map after this feed (dims = [w, h, off_x, off_y], geo = [min_x, min_y, max_x,
        max_y, ele_size, length_pixel]); footprint: the 4 plane points of the frame corners (4 x 2); M: the 3x3 homography from
        the frame to the canvas (check_M=False: one that a test injected, which need not map the frame onto the canvas points)."""
        self.grid_ = grid
        self._out = {}
        (offx, offy), (x0, y0, x1, y1), canvas, M = canvas_geometry(bgr.shape, grid, footprint, M, check_M)
        rows, cols = bgr.shape[:2]
        tx, ty = x1 - x0, y1 - y0
        self.last = ([x0 + offx, y0 + offy, tx, ty], canvas, M)

        if self._wimg is None or self._wimg.shape != (rows, cols):
            self._wimg = weight_image(rows, cols, self.weight_type)
        Minv = invert3x3(M)
        crow, ccol = ty * ELE, tx * ELE
        if self.force_float:
            src = bgr.astype(np.float32) * F(1. / 255.)                             # convertTo(CV_32FC3, 1./255.)
        else:
            src = bgr.astype(np.int16)
        xy32, xy1 = _warp_coords(Minv, crow, ccol, (32.0, 1.0))
        img = warp_linear_reflect_inv(src, Minv, crow, ccol, bool(self.force_float), xy32)
        wgt = warp_nearest_const_inv(self._wimg, Minv, crow, ccol, xy1)
        lap = create_laplace_pyr(img, self.L, self.stats if not self.force_float else None)
        wp = [wgt[:, :, None]]
        for _ in range(self.L):
            wp.append(pyr_down(wp[-1]))
        wp = [a[:, :, 0] for a in wp]

        for x in range(x0, x1):                                                     # Apply, .cpp:476-555
            for y in range(y0, y1):
                key = (x + offx, y + offy)
                t = self.tiles_.get(key)
                if t is None:
                    t = self.tiles_[key] = ([None] * (self.L + 1), [None] * (self.L + 1))
                for i in range(self.L + 1):
                    s = ELE >> i
                    sl = lap[i][(y - y0) * s:(y - y0 + 1) * s, (x - x0) * s:(x - x0 + 1) * s]
                    sw = wp[i][(y - y0) * s:(y - y0 + 1) * s, (x - x0) * s:(x - x0 + 1) * s]
                    if t[0][i] is None:                                             # fresh: a copy
                        t[0][i] = sl.copy(); t[1][i] = sw.copy()
                    else:
                        sel = sw >= t[1][i]                                         # weight-0 pixels overwrite weight-0 pixels
                        t[0][i][sel] = sl[sel]; t[1][i][sel] = sw[sel]
        return True

    # ---- what the map holds
    def tiles(self):
        return sorted(self.tiles_, key=lambda k: (k[1], k[0]))

    def tile_level(self, ix, iy, i):
        t = self.tiles_.get((ix, iy))
        return None if t is None else (t[0][i], t[1][i])

    def blend_tile_raw(self, ix, iy):
        if ("blend", ix, iy) not in self._out:
            self._out[("blend", ix, iy)] = self._blend(ix, iy)
        r = self._out[("blend", ix, iy)]
        return None if r is None else r.copy()

    def _blend(self, ix, iy):
        """Ele::blend: with all nine tiles of the 3x3 neighbourhood present (high_quality_show), each level i gets a halo of
        1 << (nl-1-i) pixels (nl = L+1 levels) from the neighbours and the collapse is cropped; otherwise the tile collapses
        alone.  Pixels whose level-0 weight is 0 are set to 0."""
        t = self.tiles_.get((ix, iy))
        if t is None:
            return None
        nl = self.L + 1
        nb = [self.tiles_.get((ix + dx, iy + dy)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        if self.high_quality and all(n is not None for n in nb):
            lv = []
            for i in range(nl):
                b, s = 1 << (nl - 1 - i), ELE >> i
                big = np.empty((s + 2 * b, s + 2 * b, 3), self.dtype)
                for yy in range(3):
                    for xx in range(3):
                        src = nb[3 * yy + xx][0][i]
                        rs = slice(s - b, s) if yy == 0 else (slice(0, s) if yy == 1 else slice(0, b))
                        cs = slice(s - b, s) if xx == 0 else (slice(0, s) if xx == 1 else slice(0, b))
                        rd = slice(0, b) if yy == 0 else (slice(b, b + s) if yy == 1 else slice(b + s, s + 2 * b))
                        cd = slice(0, b) if xx == 0 else (slice(b, b + s) if xx == 1 else slice(b + s, s + 2 * b))
                        big[rd, cd] = src[rs, cs]
                lv.append(big)
            b0 = 1 << (nl - 1)
            out = restore_from_laplace_pyr(lv)[b0:b0 + ELE, b0:b0 + ELE].copy()
        else:
            out = restore_from_laplace_pyr([a.copy() for a in t[0]])
        out[t[1][0] == 0] = 0
        return out

    def blend_tile(self, ix, iy):
        raw = self.blend_tile_raw(ix, iy)
        return None if raw is None else to_8u(raw)

    def save(self):
        if "save" not in self._out:
            self._out["save"] = self._save()
        r = self._out["save"]
        return None if r is None else (r[0].copy(), r[1])

    def _save(self):
        """save(): the bounding box of the tiles that hold a pyramid, missing tiles as zero levels, one collapse of the whole
        mosaic, the 8U view, bg_color where the level-0 weight is 0.  Returns (image, (tile x0, tile y0))."""
        if not self.tiles_:
            return None
        xs = [k[0] for k in self.tiles_]; ys = [k[1] for k in self.tiles_]
        x0, y0 = min(xs), min(ys)
        wx, wy = max(xs) + 1 - x0, max(ys) + 1 - y0
        lv = [np.zeros((wy * (ELE >> i), wx * (ELE >> i), 3), self.dtype) for i in range(self.L + 1)]
        w0 = np.zeros((wy * ELE, wx * ELE), np.float32)
        for (ix, iy), (lap, wts) in self.tiles_.items():
            for i in range(self.L + 1):
                s = ELE >> i
                lv[i][(iy - y0) * s:(iy - y0 + 1) * s, (ix - x0) * s:(ix - x0 + 1) * s] = lap[i]
            w0[(iy - y0) * ELE:(iy - y0 + 1) * ELE, (ix - x0) * ELE:(ix - x0 + 1) * ELE] = wts[0]
        out = to_8u(restore_from_laplace_pyr(lv))
        out[w0 == 0] = np.uint8(min(max(self.bg_color, 0), 255))
        return out, (x0, y0)


# ---------------------------------------------------------------- Map2DCPU: one 8-bit band, the weight in the alpha byte
# Written from Map2DFusion/Map2DCPU.cpp:236-334 and OpenCV 2.4.9's imgwarp.cpp (initInterTab2D, remapBilinear with
# FixedPtCast<int, uchar, 15>, BORDER_CONSTANT 0); shares no pixel arithmetic with oracle/oracle.c or csrc/single_band.hip.
def weight_bytes(rows, cols, weight_type):
    """The alpha plane of weightImage (.cpp:239-258): dis in float; type 0 `dis * 254.` in double, type 1 `dis * dis * 254` in float;
    the conversion to a byte truncates; then the floor of 2.  ASSUMPTION: `1 - sqrt(dis) / dis_max` is evaluated in float throughout
    (std::sqrt's float overload, as <cmath> with `using namespace std` picks it).  Were the double sqrt of <math.h> picked instead,
    the quotient would be rounded once, on the assignment to the float `dis`, and a few bytes could differ.  The oracle and the kernel
    make the same assumption, so their agreement with this function does not prove the reference's rounding."""
    xc, yc = F(cols // 2), F(rows // 2)
    dmax = np.sqrt(xc * xc + yc * yc, dtype=np.float32)
    i, j = np.mgrid[0:rows, 0:cols].astype(np.float32)
    d = (i - yc) * (i - yc) + (j - xc) * (j - xc)
    dis = F(1) - np.sqrt(d, dtype=np.float32) / dmax
    v = dis.astype(np.float64) * 254.0 if weight_type == 0 else (dis * dis * F(254)).astype(np.float64)
    return np.maximum(np.trunc(v).astype(np.uint8), np.uint8(2))


def linear_tab_fixpt(fixup=True):
    """initInterTab2D(INTER_LINEAR, fixpt = true): 32 x 32 entries (index fy, fx) of the four taps (1-fy)(1-fx), (1-fy)fx, fy(1-fx),
    fy fx as float products of the 1-D tables {1.f - x, x}, x = i * (1.f / 32), each saturate_cast<short>(v * 32768).  An entry whose
    sum is not 32768 gets the difference added to its largest (sum too small) or smallest (too large) element of the window
    k1, k2 in ksize/2 .. ksize/2 + 1: for the 2 x 2 kernel the only element of the entry in that window is (1, 1)."""
    x = np.arange(32, dtype=np.float32) * F(1.0 / 32)
    t1 = np.stack([F(1) - x, x], axis=1)                                          # interpolateLinear
    tab = np.empty((32, 32, 4), np.int64)
    for k1 in range(2):
        for k2 in range(2):
            v = (t1[:, None, k1] * t1[None, :, k2]) * F(32768)
            tab[:, :, 2 * k1 + k2] = np.clip(np.rint(v.astype(np.float64)), -32768, 32767).astype(np.int64)
    if fixup:
        diff = tab.sum(axis=2) - 32768
        tab[:, :, 3] -= diff
        tab[:, :, 3] = tab[:, :, 3].astype(np.int16)                              # the (short) cast of the fix-up
    return tab


_TAB = None


def warp_linear_const_8u_inv(src, M, drows, dcols, XY=None):
    """INTER_LINEAR + BORDER_CONSTANT(0) of an 8-bit image with the inverse map M given: sx = sat_short(X >> 5), the tap entry
    (Y & 31, X & 31); a pixel with sx >= cols, sx + 1 < 0, sy >= rows or sy + 1 < 0 is the constant; otherwise every tap outside the
    image reads 0 and the pixel is saturate_cast<uchar>((sum of v * w + (1 << 14)) >> 15), on every channel alike."""
    global _TAB
    if _TAB is None:
        _TAB = linear_tab_fixpt()
    srows, scols, cn = src.shape
    X, Y = XY if XY is not None else _warp_coords(M, drows, dcols, (32.0,))[0]
    sx = np.clip(X >> 5, -32768, 32767); sy = np.clip(Y >> 5, -32768, 32767)
    w = _TAB[Y & 31, X & 31]
    s = src.astype(np.int64)
    acc = np.zeros((drows, dcols, cn), np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        px, py = sx + dx, sy + dy
        ok = (px >= 0) & (px < scols) & (py >= 0) & (py < srows)
        v = s[np.clip(py, 0, srows - 1), np.clip(px, 0, scols - 1)]
        acc += np.where(ok[..., None], v, 0) * w[..., k, None]
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    out[(sx >= scols) | (sx + 1 < 0) | (sy >= srows) | (sy + 1 < 0)] = 0
    return out


class ModelMapSingleBand:
    """Map2DCPU (Map2D::create(TypeCPU | TypeGPU)), thread=false, one renderFrame per feed: the frame with the weight byte as its
    alpha channel is warped onto the canvas, and a stored pixel is replaced where its alpha is SMALLER than the incoming one
    (.cpp:327) -- among equal alphas the oldest keyframe stays.  Tiles are keyed by world tile like ModelMap's.

    Statistics for the tests: tie_px (pixels where an incoming alpha equalled the stored one, both > 0, summed over the feeds),
    rim_px (stored pixels with alpha 1: below the floor of 2, so interpolated with the border), and per feed the 64-column x 1-row
    blocks of the canvas whose pixels all / partly / never have 0 <= sx < cols-1 and 0 <= sy < rows-2 (waves_inside,
    waves_straddling, waves_outside)."""
    num_levels = 1

    def __init__(self, weight_type=0):
        self.weight_type = weight_type
        self.tiles_ = {}                    # (ix, iy) -> 256 x 256 x 4 uint8 (BGRA)
        self.grid_ = None
        self.last = None
        self._walpha = None
        self.tie_px = 0
        self.waves_inside = self.waves_straddling = self.waves_outside = 0

    def freeze(self):
        """no more feeds: a map that tests share (its statistics are sums over the feeds)"""
        self.frozen = True
        return self

    def feed(self, bgr, grid, footprint, M, check_M=True):
        """The arguments of ModelMap.feed; a fourth channel of the frame is ignored (the map takes the first three)."""
        assert not getattr(self, "frozen", False), "this model is shared between tests: build another one"
        self.grid_ = grid
        (offx, offy), (x0, y0, x1, y1), canvas, M = canvas_geometry(bgr.shape, grid, footprint, M, check_M)
        rows, cols = bgr.shape[:2]
        tx, ty = x1 - x0, y1 - y0
        self.last = ([x0 + offx, y0 + offy, tx, ty], canvas, M)
        if self._walpha is None or self._walpha.shape != (rows, cols):
            self._walpha = weight_bytes(rows, cols, self.weight_type)
        src = np.dstack([bgr[:, :, :3], self._walpha])                              # .cpp:266-275
        crow, ccol = ty * ELE, tx * ELE
        Minv = invert3x3(M)
        X, Y = _warp_coords(Minv, crow, ccol, (32.0,))[0]
        dst = warp_linear_const_8u_inv(src, Minv, crow, ccol, (X, Y))
        sx = np.clip(X >> 5, -32768, 32767); sy = np.clip(Y >> 5, -32768, 32767)
        ins = ((sx >= 0) & (sx < cols - 1) & (sy >= 0) & (sy < rows - 2)).reshape(crow, ccol // 64, 64)
        every, some = ins.all(axis=2), ins.any(axis=2)
        self.waves_inside += int(every.sum()); self.waves_straddling += int((some & ~every).sum())
        self.waves_outside += int((~some).sum())
        tap = [((sx + dx >= 0) & (sx + dx < cols) & (sy + dy >= 0) & (sy + dy < rows)) for dy in (0, 1) for dx in (0, 1)]
        self.last_dst = dst                                                         # the warped canvas of this feed ...
        self.last_all_taps = tap[0] & tap[1] & tap[2] & tap[3]                      # ... where all four taps lay inside the frame
        self.last_no_tap = ~(tap[0] | tap[1] | tap[2] | tap[3])                     # ... and where none did
        for x in range(x0, x1):                                                     # Apply, .cpp:308-332
            for y in range(y0, y1):
                ele = self.tiles_.get((x + offx, y + offy))
                if ele is None:
                    ele = self.tiles_[(x + offx, y + offy)] = np.zeros((ELE, ELE, 4), np.uint8)
                d = dst[(y - y0) * ELE:(y - y0 + 1) * ELE, (x - x0) * ELE:(x - x0 + 1) * ELE]
                self.tie_px += int(((ele[:, :, 3] == d[:, :, 3]) & (d[:, :, 3] > 0)).sum())
                sel = ele[:, :, 3] < d[:, :, 3]
                ele[sel] = d[sel]
        return True

    @property
    def rim_px(self):
        return sum(int((t[:, :, 3] == 1).sum()) for t in self.tiles_.values())

    def tiles(self):
        return sorted(self.tiles_, key=lambda k: (k[1], k[0]))

    def tile_bgra(self, ix, iy):
        t = self.tiles_.get((ix, iy))
        return None if t is None else t.copy()

    def blend_tile(self, ix, iy):
        t = self.tiles_.get((ix, iy))
        return None if t is None else t[:, :, :3].copy()

    def save(self):
        """The tiles' BGR pasted over their bounding box, holes zero.  Returns (image, (tile x0, tile y0)) like ModelMap.save."""
        if not self.tiles_:
            return None
        xs = [k[0] for k in self.tiles_]; ys = [k[1] for k in self.tiles_]
        x0, y0 = min(xs), min(ys)
        out = np.zeros(((max(ys) + 1 - y0) * ELE, (max(xs) + 1 - x0) * ELE, 3), np.uint8)
        for (ix, iy), t in self.tiles_.items():
            out[(iy - y0) * ELE:(iy - y0 + 1) * ELE, (ix - x0) * ELE:(ix - x0 + 1) * ELE] = t[:, :, :3]
        return out, (x0, y0)
