"""The Web-Mercator tile export restated in numpy from its description in include/pifusion.h: the OSM slippy-map formulas, the plan's
tile range and tables, the sampler's integer arithmetic after the one fp64 add, the 2 x 2 reduction over covered pixels, the pyramid with
its absent tiles.  Written from the rules, not from the kernels; no device."""
import math

import numpy as np

LD = np.longdouble


# ---------------------------------------------------------------- the globe
def lng_of_column(c, z, dtype=np.float64):
    n = dtype(256 * 2 ** z)
    return (np.asarray(c, dtype) + dtype(0.5)) / n * dtype(360) - dtype(180)


def lat_of_row(r, z, dtype=np.float64):
    n = dtype(256 * 2 ** z)
    pi = dtype(np.pi) if dtype is np.float64 else LD("3.14159265358979323846264338327950288")
    return np.arctan(np.sinh(pi * (dtype(1) - dtype(2) * (np.asarray(r, dtype) + dtype(0.5)) / n))) * dtype(180) / pi


def global_pixel(lng, lat, z):
    """continuous global pixel coordinates (x to the east, y to the south) of a position at zoom z"""
    n = 256.0 * 2 ** z
    return (lng + 180.0) / 360.0 * n, (1.0 - math.asinh(math.tan(math.radians(lat))) / math.pi) / 2.0 * n


def corners_lnglat(px2ll, rows, cols):
    p = px2ll
    return [(p[0] + p[1] * c + p[2] * r, p[3] + p[4] * c + p[5] * r) for r in (0, rows) for c in (0, cols)]


def tile_range(px2ll, rows, cols, z):
    """(tx0, ty0, tx1, ty1): the tiles the bounding box of the four image corners touches"""
    g = [global_pixel(lng, lat, z) for lng, lat in corners_lnglat(px2ll, rows, cols)]
    last = 2 ** z - 1
    t = lambda v: int(min(max(math.floor(v / 256.0), 0), last))
    return t(min(x for x, _ in g)), t(min(y for _, y in g)), t(max(x for x, _ in g)), t(max(y for _, y in g))


def tables(px2ll, rg, z, dtype=np.float64):
    """UX, UY over the global columns and VX, VY over the global rows of the range, in `dtype` arithmetic (longdouble: the reference the
    library's fp64 tables are held against)"""
    p = [dtype(v) for v in px2ll]
    det = p[1] * p[5] - p[2] * p[4]
    a00, a01, a10, a11 = p[5] / det, -p[2] / det, -p[4] / det, p[1] / det
    c = np.arange(256 * rg[0], 256 * (rg[2] + 1))
    r = np.arange(256 * rg[1], 256 * (rg[3] + 1))
    dl = lng_of_column(c, z, dtype) - p[0]
    dp = lat_of_row(r, z, dtype) - p[3]
    return a00 * dl - dtype(0.5), a10 * dl - dtype(0.5), a01 * dp, a11 * dp


def native_zoom(px2ll, rows, cols):
    lat = px2ll[3] + px2ll[4] * cols / 2.0 + px2ll[5] * rows / 2.0
    det = abs(px2ll[1] * px2ll[5] - px2ll[2] * px2ll[4])
    for z in range(25):
        if 256.0 * 2 ** z / 360.0 * math.sqrt(det / math.cos(math.radians(lat))) >= math.sqrt(0.5):
            return z
    return 24


def make_px2ll(lng, lat, rows, cols, z, scale, yaw_deg=0.0, rows_north=False):
    """a georeference whose image centre lies at (lng, lat) and whose pixels are `scale` output pixels of zoom z wide (scale > 1: the
    tiles magnify), columns pointing yaw_deg from east towards north, rows to their right (southwards at yaw 0) or to their left"""
    gsd = 156543.03392804097 * math.cos(math.radians(lat)) / 2 ** z * scale          # metres
    m_lat, m_lng = 111320.0, 111320.0 * math.cos(math.radians(lat))
    cy, sy = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    col = (gsd * cy, gsd * sy)
    row = (gsd * sy, -gsd * cy) if not rows_north else (-gsd * sy, gsd * cy)
    p1, p2, p4, p5 = col[0] / m_lng, row[0] / m_lng, col[1] / m_lat, row[1] / m_lat
    return np.array([lng - p1 * cols / 2.0 - p2 * rows / 2.0, p1, p2, lat - p4 * cols / 2.0 - p5 * rows / 2.0, p4, p5])


# ---------------------------------------------------------------- the sampler
def sample(img, mask, ux, uy, vx, vy, bg):
    """(pixels H x W x 3 uint8, covered H x W bool) for the output columns of ux / uy and rows of vx / vy"""
    rows, cols = mask.shape
    bg = min(max(int(bg), 0), 255)
    with np.errstate(invalid="ignore"):
        sx = np.asarray(ux, np.float64)[None, :] + np.asarray(vx, np.float64)[:, None]
        sy = np.asarray(uy, np.float64)[None, :] + np.asarray(vy, np.float64)[:, None]
        near = (sx > -2) & (sx < cols + 1) & (sy > -2) & (sy < rows + 1)          # false for a position that is not a number
    sx = np.where(near, sx, 0.0); sy = np.where(near, sy, 0.0)
    x0 = np.floor(sx); y0 = np.floor(sy)
    fx = np.minimum(np.floor((sx - x0) * 256.0), 255).astype(np.int64)
    fy = np.minimum(np.floor((sy - y0) * 256.0), 255).astype(np.int64)
    x0 = x0.astype(np.int64); y0 = y0.astype(np.int64)
    den = np.zeros(sx.shape, np.int64)
    acc = np.zeros(sx.shape + (3,), np.int64)
    for j in (0, 1):
        for i in (0, 1):
            x, y = x0 + i, y0 + j
            inside = near & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
            xc, yc = np.clip(x, 0, cols - 1), np.clip(y, 0, rows - 1)
            valid = inside & (mask[yc, xc] != 0)
            w = np.where(valid, (fx if i else 256 - fx) * (fy if j else 256 - fy), 0)
            den += w
            acc += w[..., None] * img[yc, xc].astype(np.int64)
    covered = 2 * den >= 65536
    d = np.maximum(den, 1)[..., None]
    px = np.where(covered[..., None], (acc + (den // 2)[..., None]) // d, bg).astype(np.uint8)
    return px, covered


def reduce4(children, bg):
    """the parent of children[j][i] = (pixels, covered) or None (absent: uncovered everywhere)"""
    bg = min(max(int(bg), 0), 255)
    big = np.zeros((512, 512, 3), np.int64); cov = np.zeros((512, 512), bool)
    for j in (0, 1):
        for i in (0, 1):
            if children[j][i] is not None:
                big[256 * j:256 * j + 256, 256 * i:256 * i + 256] = children[j][i][0]
                cov[256 * j:256 * j + 256, 256 * i:256 * i + 256] = children[j][i][1]
    n = cov.reshape(256, 2, 256, 2).sum((1, 3))
    s = (big * cov[..., None]).reshape(256, 2, 256, 2, 3).sum((1, 3))
    px = np.where((n > 0)[..., None], (s + (n >> 1)[..., None]) // np.maximum(n, 1)[..., None], bg).astype(np.uint8)
    return px, n > 0


def pyramid(img, mask, rg, ux, uy, vx, vy, zmin, zmax, bg):
    """{(z, x, y): (pixels, covered)} of every tile with a covered pixel, zmax down to zmin, from the tables of zmax over the range rg"""
    px, cov = sample(img, mask, ux, uy, vx, vy, bg)
    out, level = {}, {}
    for ty in range(rg[1], rg[3] + 1):
        for tx in range(rg[0], rg[2] + 1):
            y, x = 256 * (ty - rg[1]), 256 * (tx - rg[0])
            if cov[y:y + 256, x:x + 256].any():
                level[(tx, ty)] = (px[y:y + 256, x:x + 256], cov[y:y + 256, x:x + 256])
    for z in range(zmax, zmin - 1, -1):
        for (x, y), t in level.items():
            out[(z, x, y)] = t
        parents = {}
        for (X, Y) in sorted({(x >> 1, y >> 1) for (x, y) in level}):
            t = reduce4([[level.get((2 * X + i, 2 * Y + j)) for i in (0, 1)] for j in (0, 1)], bg)
            assert t[1].any()
            parents[(X, Y)] = t
        level = parents
    return out


def default_zmin(rg, zmax):
    """the first zoom, going down, at which the range is a single tile"""
    z = zmax
    while z > 0 and not (rg[0] >> (zmax - z) == rg[2] >> (zmax - z) and rg[1] >> (zmax - z) == rg[3] >> (zmax - z)):
        z -= 1
    return z


def cover_class(covered):
    return 2 if covered.all() else 1


def pack_mask(covered):
    """the 8192 bytes of a tile's mask: 32 a row, bit 7 of byte 0 = column 0"""
    return np.packbits(covered.astype(np.uint8), axis=1).tobytes()
