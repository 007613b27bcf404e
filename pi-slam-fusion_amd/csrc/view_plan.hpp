// view_plan.hpp -- the plan of a rendered view (view.hip, map_view.cpp, pf_render_view*): which pyramid level a view is taken from,
// which level-k pixels its four corners reach, which tiles have to be collapsed so that those pixels equal the whole-mosaic
// collapse's, and the matrix the warp runs with.  Pure host code without a device or a HIP header, as frame_plan.hpp and
// webtiles_plan.hpp: the C ABI exports it (pf_view_plan) so that the tests reach it by ctypes without a map.
//
//   V[9]       the caller's matrix, plane metres -> view pixels: (col, row, 1) ~ V (x, y, 1), in the frame of pf_grid's geo
//   A_k        level-k pixel index (relative to the first tile (tx, ty) of a region, stable tile coordinates) -> plane metres:
//                  x = lp 2^k j + min.x + (tx - off_x) eleSize,   y = lp 2^k i + min.y + (ty - off_y) eleSize
//              (a level-0 index i lies at origin + i lp, a level-k index j over level-0 index 2^k j: pyrDown samples even indices)
//   M0         V A_k, a plain triple loop in fp64: what cv::warpPerspective is handed; Minv = invert3x3(M0) is what it runs with
//   window     the level-k pixels between the source positions of the view's four corners, plus one for the second tap, clipped
//              to the content's extent: every tap that can carry weight lies in it (the preimage of a rectangle under a homography
//              whose denominator keeps its sign is a convex quadrilateral)
//   rect       the tiles the window depends on: level_step's recurrence from level k up to the top, the union of the tiles touched
//              at any level, clipped to the extent.  An edge of the rectangle is either an edge of the extent -- where pyrUp's edge
//              forms are the right ones -- or lies beyond everything a window pixel depends on, so the window's pixels of the
//              rectangle's collapse are those of the whole mosaic's
#pragma once
#include "../../include/pifusion.h"
#include "geometry.hpp"
#include "level_step.hpp"
#include "plan_limits.hpp"
#include "webtiles_plan.hpp"
#include <cmath>
#include <cstring>

namespace pf {
namespace view {

constexpr int kMaxViewDim = 16384;
constexpr int kMaxRegion = 32767;               // sat_short's range: the warp's source coordinates are shorts

enum PlanResult { kOk = 0, kArguments, kNotFinite, kSize, kLevel, kSingular, kHorizon, kRegion };

inline const char* plan_message(PlanResult r)
{
    switch (r) {
    case kArguments: return "no matrix, no grid or no result";
    case kNotFinite: return "the matrix V is not finite";
    case kSize: return "width and height must lie in 1 .. 16384";
    case kLevel: return "the level is outside -1 .. the map's top level";
    case kSingular: return "the matrix from level pixels to view pixels is singular";
    case kHorizon: return "the denominator is zero or changes sign over the view's corners (the horizon lies inside the view)";
    case kRegion: return "the view needs a region of more than 32767 pixels a side at this level: ask for a higher level";
    default: return "ok";
    }
}

// A_k for a region whose first tile is (tx, ty); dims = {w, h, off_x, off_y}, geo = {min.x, min.y, max.x, max.y, eleSize, lengthPixel}
inline void level_to_plane(int k, int tx, int ty, const int dims[4], const double geo[6], double A[9])
{
    const double s = geo[5] * (double)(1 << k);
    A[0] = s; A[1] = 0; A[2] = geo[0] + (tx - dims[2]) * geo[4];
    A[3] = 0; A[4] = s; A[5] = geo[1] + (ty - dims[3]) * geo[4];
    A[6] = 0; A[7] = 0; A[8] = 1;
}

inline void mul3x3(const double P[9], const double Q[9], double R[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s = s + P[i * 3 + k] * Q[k * 3 + j];
            R[i * 3 + j] = s;
        }
}

// the level of `level = -1`: s = sqrt |det J| of (view pixel -> level-0 pixel) at the view's centre, k = floor(log2(max(s, 1)))
// clamped to 0 .. L -- by comparison against the powers of two, so that a dyadic s falls on the right side of each
inline PlanResult choose_level(const double V[9], int width, int height, const int dims[4], const double geo[6], int L, int* level)
{
    double A[9], M0[9], M[9];
    level_to_plane(0, dims[2], dims[3], dims, geo, A);          // the origin does not enter the Jacobian
    mul3x3(V, A, M0);
    if (!invert3x3(M0, M)) return kSingular;
    const double cx = (width - 1) * 0.5, cy = (height - 1) * 0.5;
    const double X = M[0] * cx + M[1] * cy + M[2], Y = M[3] * cx + M[4] * cy + M[5], W = M[6] * cx + M[7] * cy + M[8];
    if (!(W != 0) || !std::isfinite(W)) return kHorizon;
    const double w2 = W * W;
    const double xu = (M[0] * W - X * M[6]) / w2, xv = (M[1] * W - X * M[7]) / w2, yu = (M[3] * W - Y * M[6]) / w2, yv = (M[4] * W - Y * M[7]) / w2;
    const double s = std::sqrt(std::fabs(xu * yv - xv * yu));
    if (!std::isfinite(s)) return kSingular;
    int k = 0;
    while (k < L && s >= (double)(2 << k)) k++;
    *level = k;
    return kOk;
}

// dims, geo: pf_grid's; extent = {tx0, ty0, tiles across, tiles down} of the content in stable tile coordinates (across or down 0:
// no content).  On a refusal nothing is written
inline PlanResult plan(const double V[9], int width, int height, int level, const int dims[4], const double geo[6], int num_levels, const int extent[4], pf_view_info* out)
{
    if (!V || !dims || !geo || !extent || !out || num_levels < 1 || num_levels > kMaxLevels) return kArguments;
    for (int i = 0; i < 9; i++) if (!std::isfinite(V[i])) return kNotFinite;
    for (int i = 0; i < 6; i++) if (!std::isfinite(geo[i])) return kArguments;
    if (width < 1 || width > kMaxViewDim || height < 1 || height > kMaxViewDim) return kSize;
    const int L = num_levels - 1;
    if (level < -1 || level > L) return kLevel;
    int k = level;
    if (level < 0) { const PlanResult r = choose_level(V, width, height, dims, geo, L, &k); if (r != kOk) return r; }
    const bool content = extent[2] > 0 && extent[3] > 0;
    const int ex = content ? extent[0] : dims[2], ey = content ? extent[1] : dims[3];
    pf_view_info v;
    std::memset(&v, 0, sizeof v);
    v.level = k;
    // against the extent's origin first: the corners' source positions, the horizon
    double A[9];
    level_to_plane(k, ex, ey, dims, geo, A);
    mul3x3(V, A, v.M0);
    if (!invert3x3(v.M0, v.Minv)) return kSingular;
    const double* M = v.Minv;
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    int sign = 0;
    for (int c = 0; c < 4; c++) {
        const double u = (c & 1) ? (double)(width - 1) : 0.0, w = (c & 2) ? (double)(height - 1) : 0.0;
        const double X = M[0] * u + M[1] * w + M[2], Y = M[3] * u + M[4] * w + M[5], W = M[6] * u + M[7] * w + M[8];
        if (!(W != 0) || !std::isfinite(W)) return kHorizon;
        const int s = W > 0 ? 1 : -1;
        if (sign && s != sign) return kHorizon;
        sign = s;
        const double fx = X / W, fy = Y / W;
        if (!std::isfinite(fx) || !std::isfinite(fy)) return kHorizon;
        if (!c) { x0 = x1 = fx; y0 = y1 = fy; }
        x0 = fx < x0 ? fx : x0; x1 = fx > x1 ? fx : x1; y0 = fy < y0 ? fy : y0; y1 = fy > y1 ? fy : y1;
    }
    v.empty = 1;
    if (!content) { *out = v; return kOk; }
    // the window in level-k pixels of the extent: floor(min) .. floor(max) + 1, clipped
    const int e = kElePixels >> k;
    const long long cols = (long long)extent[2] * e, rows = (long long)extent[3] * e;
    auto lo_of = [](double f, long long n) { const double g = std::floor(f); return g < 0 ? 0ll : (g > (double)n ? n : (long long)g); };
    auto hi_of = [](double f, long long n) { const double g = std::floor(f) + 1; return g < -1 ? -1ll : (g > (double)(n - 1) ? n - 1 : (long long)g); };
    const long long wx0 = lo_of(x0, cols), wx1 = hi_of(x1, cols), wy0 = lo_of(y0, rows), wy1 = hi_of(y1, rows);
    if (wx0 > wx1 || wy0 > wy1) { *out = v; return kOk; }          // the view misses the extent
    // tiles touched at level k, then level_step's recurrence up to the top; tiles at level i hold 256 >> i pixels a side
    long long tx0 = wx0 / e, tx1 = wx1 / e, ty0 = wy0 / e, ty1 = wy1 / e;
    if ((tx1 - tx0 + 1) * e > kMaxRegion || (ty1 - ty0 + 1) * e > kMaxRegion) return kRegion;          // (before ints are made of the window)
    int xl = (int)wx0, xh = (int)wx1, yl = (int)wy0, yh = (int)wy1;
    if (cols > 0x7fffffffll || rows > 0x7fffffffll) return kRegion;
    for (int i = k + 1; i <= L; i++) {
        level_step(xl, xh, (int)(cols >> (i - k)));
        level_step(yl, yh, (int)(rows >> (i - k)));
        const int ei = kElePixels >> i;
        tx0 = xl / ei < tx0 ? xl / ei : tx0; tx1 = xh / ei > tx1 ? xh / ei : tx1;
        ty0 = yl / ei < ty0 ? yl / ei : ty0; ty1 = yh / ei > ty1 ? yh / ei : ty1;
    }
    const int across = (int)(tx1 - tx0 + 1), down = (int)(ty1 - ty0 + 1);
    if ((long long)across * e > kMaxRegion || (long long)down * e > kMaxRegion) return kRegion;
    v.empty = 0;
    v.rect[0] = ex + (int)tx0; v.rect[1] = ey + (int)ty0; v.rect[2] = across; v.rect[3] = down;
    v.tiles = across * down;
    v.window[0] = (int)(wx0 - tx0 * e); v.window[1] = (int)(wy0 - ty0 * e); v.window[2] = (int)(wx1 - wx0 + 1); v.window[3] = (int)(wy1 - wy0 + 1);
    // the matrix against the rectangle's origin: what the warp runs with
    level_to_plane(k, v.rect[0], v.rect[1], dims, geo, A);
    mul3x3(V, A, v.M0);
    if (!invert3x3(v.M0, v.Minv)) return kSingular;
    *out = v;
    return kOk;
}

// ---- helpers that only make a V (pf_view_of_extent, pf_view_from_pose, pf_view_from_lnglat)

// plane metres -> continuous level-0 pixel coordinate (index + 0.5) relative to plane point (ox, oy)
inline void plane_to_continuous(double ox, double oy, double lp, double C[9])
{
    C[0] = 1. / lp; C[1] = 0; C[2] = 0.5 - ox / lp;
    C[3] = 0; C[4] = 1. / lp; C[5] = 0.5 - oy / lp;
    C[6] = 0; C[7] = 0; C[8] = 1;
}

// the whole content in width x height: axes as the map's, aspect kept, centred; pixels as areas, so the extent's outer corners fall
// on the view's where the aspects agree
inline bool of_extent(const int dims[4], const double geo[6], const int extent[4], int width, int height, double V[9])
{
    if (extent[2] <= 0 || extent[3] <= 0 || width < 1 || height < 1) return false;
    const double cols = (double)extent[2] * kElePixels, rows = (double)extent[3] * kElePixels;
    const double sx = width / cols, sy = height / rows, s = sx < sy ? sx : sy;
    double C[9];
    plane_to_continuous(geo[0] + (extent[0] - dims[2]) * geo[4], geo[1] + (extent[1] - dims[3]) * geo[4], geo[5], C);
    const double U[9] = { s, 0, (width - s * cols) * 0.5 - 0.5, 0, s, (height - s * rows) * 0.5 - 0.5, 0, 0, 1 };
    mul3x3(U, C, V);
    return true;
}

// what a camera at `pose` (plane coordinates) sees: footprint's four plane points to the image corners, in double
inline bool from_pose(const Camera& c, const Pose& pose, double V[9])
{
    double pts[8];
    if (!footprint(c, pose, pts)) return false;
    const double img[8] = { 0, 0, c.w, 0, 0, c.h, c.w, c.h };
    perspective_transform(pts, img, V);
    return true;
}

// a north-up window linear in degrees: (lng_w, lat_n) at the continuous view coordinate (0, 0), (lng_e, lat_s) at (width, height);
// plane metres -> continuous level-0 pixel -> degrees (pf_webtiles_georef's chain for a mosaic whose first pixel lies at the grid's
// minimum) -> continuous view coordinate -> view pixel index
inline bool from_lnglat(const double geo[6], const double plane7[7], const double gps_origin[3], double lng_w, double lat_n, double lng_e, double lat_s, int width, int height,
                        double V[9])
{
    if (width < 1 || height < 1 || !(lng_e != lng_w) || !(lat_s != lat_n)) return false;
    double T[16] = {};
    T[0] = geo[5]; T[3] = geo[0]; T[5] = geo[5]; T[7] = geo[1]; T[10] = 1; T[15] = 1;
    double p[6];
    webtiles::georef_compose(T, plane7, gps_origin, p);
    if (!webtiles::finite6(p)) return false;
    double C[9], PC[9], U[9];
    plane_to_continuous(geo[0], geo[1], geo[5], C);
    const double P[9] = { p[1], p[2], p[0], p[4], p[5], p[3], 0, 0, 1 };
    const double ax = width / (lng_e - lng_w), ay = height / (lat_s - lat_n);
    U[0] = ax; U[1] = 0; U[2] = -lng_w * ax - 0.5; U[3] = 0; U[4] = ay; U[5] = -lat_n * ay - 0.5; U[6] = 0; U[7] = 0; U[8] = 1;
    mul3x3(P, C, PC);
    mul3x3(U, PC, V);
    for (int i = 0; i < 9; i++) if (!std::isfinite(V[i])) return false;
    return true;
}

}  // namespace view
}  // namespace pf
