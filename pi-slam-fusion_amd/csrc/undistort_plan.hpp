// undistort_plan.hpp -- the host side of keyframe undistortion: GSLAM's three camera models, the remap table from a distorted input
// camera into the map's pinhole camera, and the search for an output camera that the input covers.  Pure host code, no HIP.
//
// The table is what UndistorterImpl::prepareReMap (GSLAM/core/Undistorter.h:85-168) leaves in remapX / remapY: for every output pixel
// (x, y), P = out.UnProject(x, y) and q = in.Project(P) in double, with the operations and the operation order of the portable (non-SSE3)
// branches of GSLAM/core/Camera.h.  Every translation unit that includes this header is compiled with floating-point contraction off
// (the Makefile's -ffp-contract=off), so a product and the sum that takes it are rounded one after the other, as on x86-64 SSE2.
#pragma once
#include <cmath>
#include <cstddef>

namespace pf {
namespace undistort {

struct InCamera {
    enum Kind { PinHole = 6, ATAN = 7, OpenCV = 11 };
    int    kind = 0, w = 0, h = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0;
    double d = 0, d_inv = 0, tan2w = 0;             // ATAN
    bool   use_distortion = false;
    double k1 = 0, k2 = 0, p1 = 0, p2 = 0, k3 = 0;  // OpenCV
};

// Camera::Camera(std::vector<double>) (Camera.h:407-416) for n = 6, 7, 11; false for any other n and for a camera that is not isValid()
// (w, h > 0 after the (int) conversion, fx, fy != 0) or not finite
inline bool make_camera(const double* p, int n, InCamera& c)
{
    if (!p || (n != 6 && n != 7 && n != 11)) return false;
    for (int i = 0; i < n; i++) if (!std::isfinite(p[i])) return false;
    if (!(p[0] >= 1 && p[0] < 65536 && p[1] >= 1 && p[1] < 65536)) return false;
    c = InCamera();
    c.kind = n; c.w = (int)p[0]; c.h = (int)p[1];
    c.fx = p[2]; c.fy = p[3]; c.cx = p[4]; c.cy = p[5];
    if (c.fx == 0 || c.fy == 0) return false;
    if (n == 7) {
        c.d = p[6];
        // CameraATAN::refreshParaments (:230-233): intrinsics given as fractions of the image size
        if (c.fx < 1 && c.fy < 1) { c.fx *= c.w; c.fy *= c.h; c.cx *= c.w; c.cy *= c.h; }
        if (c.fx == 0 || c.fy == 0) return false;
        if (c.d != 0.0) { c.tan2w = 2.0 * std::tan(c.d / 2.0); c.d_inv = 1.0 / c.d; c.use_distortion = true; }
    } else if (n == 11) {
        c.k1 = p[6]; c.k2 = p[7]; c.p1 = p[8]; c.p2 = p[9]; c.k3 = p[10];
    }
    return true;
}

// the output camera: the six numbers of pf_prepare
struct OutCamera { int w, h; double fx, fy, cx, cy, fx_inv, fy_inv; };
inline bool make_out_camera(const double* p, OutCamera& o)
{
    if (!p) return false;
    for (int i = 0; i < 6; i++) if (!std::isfinite(p[i])) return false;
    if (!(p[0] >= 1 && p[0] < 65536 && p[1] >= 1 && p[1] < 65536) || p[2] == 0 || p[3] == 0) return false;
    o.w = (int)p[0]; o.h = (int)p[1]; o.fx = p[2]; o.fy = p[3]; o.cx = p[4]; o.cy = p[5];
    o.fx_inv = 1. / o.fx; o.fy_inv = 1. / o.fy;
    return true;
}

// in.Project(Point3d(X, Y, 1.)): the z == 1 paths of Camera.h:201-204, :296-311, :358-379
inline void project(const InCamera& c, double X, double Y, double& u, double& v)
{
    if (c.kind == InCamera::OpenCV) {
        double r2, r4, r6, X1, Y1, X2, Y2, xy2;
        X2 = X * X;
        Y2 = Y * Y;
        r2 = X2 + Y2;
        r4 = r2 * r2;
        r6 = r2 * r4;
        xy2 = X * Y * 2.0;
        X1 = X * (1. + c.k1 * r2 + c.k2 * r4 + c.k3 * r6) + xy2 * c.p1 + c.p2 * (r2 + 2.0 * X2);
        Y1 = Y * (1. + c.k1 * r2 + c.k2 * r4 + c.k3 * r6) + xy2 * c.p2 + c.p1 * (r2 + 2.0 * Y2);
        u = c.cx + c.fx * X1; v = c.cy + c.fy * Y1;
    } else if (c.kind == InCamera::ATAN && c.use_distortion) {
        double r = std::sqrt(X * X + Y * Y);
        if (r < 0.001 || c.d == 0.0) r = 1.0;
        else r = (c.d_inv * std::atan(r * c.tan2w) / r);
        u = c.cx + c.fx * r * X; v = c.cy + c.fy * r * Y;
    } else {
        u = c.fx * X + c.cx; v = c.fy * Y + c.cy;
    }
}

// one entry: false (and (-1, -1)) when the output pixel looks past the input image -- the test is on the doubles
inline bool entry(const InCamera& in, const OutCamera& out, int x, int y, float& tx, float& ty)
{
    const double X = ((double)x - out.cx) * out.fx_inv, Y = ((double)y - out.cy) * out.fy_inv;
    double u, v;
    project(in, X, Y, u, v);
    if (u < 0 || v < 0 || u >= in.w || v >= in.h || u != u || v != v) { tx = -1.f; ty = -1.f; return false; }
    tx = (float)u; ty = (float)v;
    return true;
}

// the whole table, row-major, out.w * out.h entries in each of x and y (either may be null); returns the number of uncovered entries
inline long long build_table(const InCamera& in, const OutCamera& out, float* x, float* y)
{
    long long uncovered = 0;
    for (int r = 0; r < out.h; r++)
        for (int c = 0; c < out.w; c++) {
            float tx, ty;
            if (!entry(in, out, c, r, tx, ty)) uncovered++;
            const size_t i = (size_t)r * out.w + c;
            if (x) x[i] = tx;
            if (y) y[i] = ty;
        }
    return uncovered;
}

// every pixel of the output image's four border lines has a valid entry
inline bool border_covered(const InCamera& in, const OutCamera& out)
{
    float tx, ty;
    for (int c = 0; c < out.w; c++) if (!entry(in, out, c, 0, tx, ty) || !entry(in, out, c, out.h - 1, tx, ty)) return false;
    for (int r = 0; r < out.h; r++) if (!entry(in, out, 0, r, tx, ty) || !entry(in, out, out.w - 1, r, tx, ty)) return false;
    return true;
}

constexpr int kFitUnit = 4096, kFitMax = 64 * 4096;

inline OutCamera scaled(const OutCamera& want, int k)
{
    OutCamera o = want;
    const double s = (double)k / kFitUnit;
    o.fx = s * want.fx; o.fy = s * want.fy; o.fx_inv = 1. / o.fx; o.fy_inv = 1. / o.fy;
    return o;
}

// w, h, cx, cy of `want` kept: the smallest k >= 4096 (s = k / 4096 >= 1) at which the output camera (s fx, s fy) has its whole border
// covered, found by bisection between an uncovered k and a covered one (the border's coverage grows with the focal length for every lens
// whose distortion is monotone over the field of view: zooming in pulls the border towards the centre).  0: none up to s = 64
inline int fit_scale(const InCamera& in, const OutCamera& want)
{
    if (border_covered(in, scaled(want, kFitUnit))) return kFitUnit;
    int lo = kFitUnit, hi = 2 * kFitUnit;           // lo: uncovered
    while (hi <= kFitMax && !border_covered(in, scaled(want, hi))) { lo = hi; hi *= 2; }
    if (hi > kFitMax) return 0;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (border_covered(in, scaled(want, mid))) hi = mid; else lo = mid;
    }
    return hi;
}

}  // namespace undistort
}  // namespace pf
