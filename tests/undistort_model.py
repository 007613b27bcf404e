"""Numpy model of keyframe undistortion (DESIGN.md "Undistortion") -- test code only, standing alone: no library call, no shared code.

The table: for every output pixel (x, y), P = out.UnProject(x, y) and q = in.Project(P) in float64 with the operations and the operation
order of the portable branches of GSLAM/core/Camera.h; (-1, -1) where q lies outside [0, w_in) x [0, h_in), tested on the doubles;
otherwise (float32(q.x), float32(q.y)).  numpy rounds every float64 operation once, as SSE2 does, so products and sums written one
after the other here are the reference's.

The pixel: UndistorterImpl::undistort's colour branch in float32, summed left to right, truncated -- with the three deviations of
DESIGN.md: taps clamped into the source, an entry with X < 0 black, no nearest variant.

table() and pixels() take switches that turn single rules off; tests/test_undistort_model.py uses them to show that its comparisons
notice (a mutation check, as tests/warp_ties.py does for the warp)."""
import math

import numpy as np

F = np.float32


def in_camera(p):
    """the parameters as Camera::Camera(std::vector<double>) and the models' constructors leave them: dict with kind 6 / 7 / 11"""
    p = [float(v) for v in p]
    assert len(p) in (6, 7, 11)
    c = dict(kind=len(p), w=int(p[0]), h=int(p[1]), fx=p[2], fy=p[3], cx=p[4], cy=p[5])
    if len(p) == 7:
        c["d"] = p[6]
        if c["fx"] < 1 and c["fy"] < 1:             # CameraATAN::refreshParaments: intrinsics as fractions of the image size
            c["fx"] *= c["w"]; c["fy"] *= c["h"]; c["cx"] *= c["w"]; c["cy"] *= c["h"]
    if len(p) == 11:
        c.update(k1=p[6], k2=p[7], p1=p[8], p2=p[9], k3=p[10])
    return c


def project(c, X, Y):
    """in.Project(Point3d(X, Y, 1)) on float64 arrays"""
    fx, fy, cx, cy = c["fx"], c["fy"], c["cx"], c["cy"]
    if c["kind"] == 11:
        k1, k2, p1, p2, k3 = c["k1"], c["k2"], c["p1"], c["p2"], c["k3"]
        X2 = X * X
        Y2 = Y * Y
        r2 = X2 + Y2
        r4 = r2 * r2
        r6 = r2 * r4
        xy2 = X * Y * 2.0
        X1 = X * (1. + k1 * r2 + k2 * r4 + k3 * r6) + xy2 * p1 + p2 * (r2 + 2.0 * X2)
        Y1 = Y * (1. + k1 * r2 + k2 * r4 + k3 * r6) + xy2 * p2 + p1 * (r2 + 2.0 * Y2)
        return cx + fx * X1, cy + fy * Y1
    if c["kind"] == 7 and c["d"] != 0.0:
        d = c["d"]
        tan2w = 2.0 * math.tan(d / 2.0)
        d_inv = 1.0 / d
        r = np.sqrt(X * X + Y * Y)
        small = r < 0.001
        f = np.where(small, 1.0, d_inv * np.arctan(r * tan2w) / np.where(small, 1.0, r))
        return cx + fx * f * X, cy + fy * f * Y
    return fx * X + cx, fy * Y + cy


def coordinates(cam_in, cam_out):
    """(u, v, valid): the float64 coordinates of every output pixel in the input image and the reference's validity test on them"""
    c = in_camera(cam_in)
    w, h, fx, fy, cx, cy = [float(v) for v in cam_out]
    w, h = int(w), int(h)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = (xs - cx) * (1. / fx)
    Y = (ys - cy) * (1. / fy)
    u, v = project(c, X, Y)
    valid = ~((u < 0) | (v < 0) | (u >= c["w"]) | (v >= c["h"]))
    return u, v, valid


def table(cam_in, cam_out):
    """(x, y, uncovered): float32 h x w each"""
    u, v, valid = coordinates(cam_in, cam_out)
    x = np.where(valid, u, -1.0).astype(F)
    y = np.where(valid, v, -1.0).astype(F)
    return x, y, int((~valid).sum())


def pixels(x, y, src, truncate=True, clamp=True, valid_rule="ge0"):
    """The undistorted BGR frame of src (h_in x w_in x 3 or x 4 uint8; alpha ignored) through table (x, y).
    Mutations: truncate=False rounds to nearest; clamp=False wraps a tap past the last column / row to the first one (the reference reads the
    next row's first pixel, or past the buffer); valid_rule="gt0" is the reference's colour-branch slip, X > 0."""
    src = np.asarray(src)
    h_in, w_in = src.shape[:2]
    x = np.asarray(x, F); y = np.asarray(y, F)
    xi = x.astype(np.int32); yi = y.astype(np.int32)
    xx = (x - xi.astype(F)).astype(F); yy = (y - yi.astype(F)).astype(F)
    xy = (xx * yy).astype(F)
    one = F(1)
    c0 = (((one - xx).astype(F) - yy).astype(F) + xy).astype(F)
    c1 = (xx - xy).astype(F); c2 = (yy - xy).astype(F); c3 = xy
    if clamp:
        x0 = np.clip(xi, 0, w_in - 1); x1 = np.clip(xi + 1, 0, w_in - 1)
        y0 = np.clip(yi, 0, h_in - 1); y1 = np.clip(yi + 1, 0, h_in - 1)
    else:
        x0 = xi % w_in; x1 = (xi + 1) % w_in
        y0 = yi % h_in; y1 = (yi + 1) % h_in
    ok = (x > 0) if valid_rule == "gt0" else ~(x < 0)
    out = np.zeros(x.shape + (3,), np.uint8)
    for j in range(3):
        p = src[:, :, j].astype(F)
        s = (p[y0, x0] * c0).astype(F)
        s = (s + (p[y0, x1] * c1).astype(F)).astype(F)
        s = (s + (p[y1, x0] * c2).astype(F)).astype(F)
        s = (s + (p[y1, x1] * c3).astype(F)).astype(F)
        if not truncate:
            s = np.floor(s.astype(np.float64) + 0.5)
        out[:, :, j] = np.where(ok, s.astype(np.int32) & 255, 0).astype(np.uint8)
    return out


def undistort(src, cam_in, cam_out, **kw):
    x, y, _ = table(cam_in, cam_out)
    return pixels(x, y, src, **kw)


def source_frame(rows, cols, seed, cn=3):
    """deterministic noise, every byte value"""
    return np.random.RandomState(seed).randint(0, 256, (rows, cols, cn)).astype(np.uint8)
