// webtiles_plan.hpp -- the georeference and the sampling plan of the Web-Mercator tile export (webtiles.hip, pf_webtiles*): where
// a mosaic pixel lies on the globe, which XYZ tiles (EPSG:3857, the OSM slippy-map numbering) its extent touches at a zoom, and
// the four tables of doubles that take an output pixel of those tiles back to a source position.  Pure host code without a device
// or a HIP header, as frame_plan.hpp: the C ABI exports it (pf_webtiles_plan, pf_webtiles_native_zoom, pf_webtiles_georef_compose)
// so that the tests reach it by ctypes.
//
//   px2ll[6]   the affine from a CONTINUOUS mosaic pixel coordinate (column, row) to degrees:
//                  lng = P0 + P1 col + P2 row,   lat = P3 + P4 col + P5 row
//              pixel (i, j) covers [i, i + 1) x [j, j + 1), its centre lies at + 0.5 (RasterPixelIsArea, as the TIFF declares)
//   zoom z     n = 256 * 2^z global pixels a side; global pixel column c and row r have their centres at
//                  lng_c = (c + 0.5) / n * 360 - 180,   lat_r = atan(sinh(pi (1 - 2 (r + 0.5) / n))) * 180 / pi
//   tables     with A = inverse of [[P1 P2] [P4 P5]]:  UX[c] = A00 (lng_c - P0) - 0.5,  VX[r] = A01 (lat_r - P3),
//                                                      UY[c] = A10 (lng_c - P0) - 0.5,  VY[r] = A11 (lat_r - P3)
//              output pixel (c, r) samples the source at sx = UX[c] + VX[r], sy = UY[c] + VY[r] in pixel-index coordinates (the
//              centre of pixel i at i): one fp64 add each, which the kernel repeats exactly (-ffp-contract=off)
#pragma once
#include "geometry.hpp"
#include <algorithm>
#include <cmath>

namespace pf {
namespace webtiles {

constexpr int kMaxZoom = 24;                    // 256 * 2^24 = 2^32 global pixels: columns and rows still fit 64-bit arithmetic with room
constexpr double kMaxLat = 85.05;               // the square Mercator world ends at 85.0511 degrees
constexpr double kPi = 3.14159265358979323846;

// metres per degree of longitude and latitude at latitude lat1: the two divisors of pf_lnglat_from_distance, by the same operations
inline void lnglat_units(double lat1, double* lng_unit, double* lat_unit)
{
    const double kEarthRadius = 6378137.0, kDeg2Rad = 0.017453292519943;
    const double a = kEarthRadius, f = 1.0 / 298.257223563, e_2 = 2 * f - f * f;
    const double phi_rad = lat1 * kDeg2Rad;
    const double sp = std::sin(phi_rad);
    *lng_unit = kDeg2Rad * a * std::cos(phi_rad) / std::sqrt(1 - e_2 * (sp * sp));
    *lat_unit = kDeg2Rad * a * (1 - e_2) / std::pow(1 - e_2 * (sp * sp), 1.5);
}

// pf_webtiles_georef's chain: pixel -> plane metres (transform: the 16 doubles of the TIFF's ModelTransformationTag) -> world
// (plane pose: world = t + R (x, y, 0), East = world.x, North = world.y, as pf_format_map_update) -> degrees around gps_origin
// (pf_lnglat_from_distance: linear in East and North).  Exactly affine
inline void georef_compose(const double transform[16], const double plane7[7], const double gps_origin[3], double px2ll[6])
{
    double lng_unit, lat_unit;
    lnglat_units(gps_origin[1], &lng_unit, &lat_unit);
    const Pose pl = pose_from7(plane7);
    const double ex[3] = { 1, 0, 0 }, ey[3] = { 0, 1, 0 };
    double rx[3], ry[3];
    rotate(pl.q, ex, rx); rotate(pl.q, ey, ry);
    // plane metres of pixel (col, row): x = T0 col + T1 row + T3, y = T4 col + T5 row + T7
    const double x0 = transform[3], xc = transform[0], xr = transform[1], y0 = transform[7], yc = transform[4], yr = transform[5];
    const double e0 = pl.t[0] + rx[0] * x0 + ry[0] * y0, ec = rx[0] * xc + ry[0] * yc, er = rx[0] * xr + ry[0] * yr;
    const double n0 = pl.t[1] + rx[1] * x0 + ry[1] * y0, nc = rx[1] * xc + ry[1] * yc, nr = rx[1] * xr + ry[1] * yr;
    px2ll[0] = e0 / lng_unit + gps_origin[0]; px2ll[1] = ec / lng_unit; px2ll[2] = er / lng_unit;
    px2ll[3] = n0 / lat_unit + gps_origin[1]; px2ll[4] = nc / lat_unit; px2ll[5] = nr / lat_unit;
}

inline bool finite6(const double p[6]) { for (int i = 0; i < 6; i++) if (!std::isfinite(p[i])) return false; return true; }

// the inverse of the 2 x 2 part; false when it is singular (a vertical plane) or not finite
inline bool invert2(const double px2ll[6], double A[4])
{
    if (!finite6(px2ll)) return false;
    const double a = px2ll[1], b = px2ll[2], c = px2ll[4], d = px2ll[5], det = a * d - b * c;
    const double scale = std::max(std::max(std::fabs(a), std::fabs(b)), std::max(std::fabs(c), std::fabs(d)));
    if (!(scale > 0) || !(std::fabs(det) > 1e-12 * scale * scale)) return false;
    A[0] = d / det; A[1] = -b / det; A[2] = -c / det; A[3] = a / det;
    return true;
}

inline double global_x(double lng, double n) { return (lng + 180.0) / 360.0 * n; }
inline double global_y(double lat, double n) { return (1.0 - std::asinh(std::tan(lat * kPi / 180.0)) / kPi) / 2.0 * n; }
inline double lng_of_column(double c, double n) { return (c + 0.5) / n * 360.0 - 180.0; }
inline double lat_of_row(double r, double n) { return std::atan(std::sinh(kPi * (1.0 - 2.0 * (r + 0.5) / n))) * 180.0 / kPi; }

enum PlanResult { kPlanOk = 0, kPlanBadZoom, kPlanSingular, kPlanLatitude, kPlanCapacity, kPlanArguments };

// the inclusive tile range {tx0, ty0, tx1, ty1} that the bounding box of the four image corners touches at zoom z
inline PlanResult tile_range(const double px2ll[6], int rows, int cols, int z, int range[4])
{
    if (!px2ll || !range || rows < 1 || cols < 1) return kPlanArguments;
    if (z < 0 || z > kMaxZoom) return kPlanBadZoom;
    double A[4];
    if (!invert2(px2ll, A)) return kPlanSingular;
    const double n = 256.0 * (double)(1ll << z);
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    for (int k = 0; k < 4; k++) {
        const double c = (k & 1) ? (double)cols : 0.0, r = (k & 2) ? (double)rows : 0.0;
        const double lng = px2ll[0] + px2ll[1] * c + px2ll[2] * r, lat = px2ll[3] + px2ll[4] * c + px2ll[5] * r;
        if (!(std::fabs(lat) <= kMaxLat) || !std::isfinite(lng)) return kPlanLatitude;
        const double gx = global_x(lng, n), gy = global_y(lat, n);
        if (!k) { x0 = x1 = gx; y0 = y1 = gy; }
        x0 = std::min(x0, gx); x1 = std::max(x1, gx); y0 = std::min(y0, gy); y1 = std::max(y1, gy);
    }
    const double last = (double)((1ll << z) - 1);
    auto tile = [&](double g) { const double t = std::floor(g / 256.0); return (int)(t < 0 ? 0 : t > last ? last : t); };
    range[0] = tile(x0); range[1] = tile(y0); range[2] = tile(x1); range[3] = tile(y1);
    return kPlanOk;
}

// range and tables of zoom z; ux / uy hold 256 (tx1 - tx0 + 1) doubles from global column 256 tx0 on, vx / vy 256 (ty1 - ty0 + 1)
// from global row 256 ty0 on.  Tables that are too small (cap_cols, cap_rows: doubles each of the two pairs can take) are left alone
// and the range alone is reported: it says how many are needed, as pf_dist_plan_blend reports its counts.  Every other refusal
// writes nothing.  Without any table (four null pointers) the call asks for the range only and succeeds
inline PlanResult plan(const double px2ll[6], int rows, int cols, int z, int range[4], double* ux, double* uy, double* vx, double* vy, long long cap_cols, long long cap_rows)
{
    int rg[4];
    const PlanResult r = tile_range(px2ll, rows, cols, z, rg);
    if (r != kPlanOk) return r;
    const long long nc = 256ll * (rg[2] - rg[0] + 1), nr = 256ll * (rg[3] - rg[1] + 1);
    for (int k = 0; k < 4; k++) range[k] = rg[k];
    if (!ux && !uy && !vx && !vy) return kPlanOk;          // a question: the range alone
    if (nc > cap_cols || nr > cap_rows || !ux || !uy || !vx || !vy) return kPlanCapacity;
    double A[4];
    invert2(px2ll, A);
    const double n = 256.0 * (double)(1ll << z);
    for (long long i = 0; i < nc; i++) {
        const double d = lng_of_column((double)(256ll * rg[0] + i), n) - px2ll[0];
        ux[i] = A[0] * d - 0.5; uy[i] = A[2] * d - 0.5;
    }
    for (long long i = 0; i < nr; i++) {
        const double d = lat_of_row((double)(256ll * rg[1] + i), n) - px2ll[3];
        vx[i] = A[1] * d; vy[i] = A[3] * d;
    }
    return kPlanOk;
}

// the smallest zoom at which one source pixel spans at least 1 / sqrt 2 output pixel: sqrt |det| of d(global px) / d(source px) at
// the image centre, (n / 360) sqrt(sec(lat) |P1 P5 - P2 P4|).  -1 when the affine is singular or the centre lies past the square world
inline int native_zoom(const double px2ll[6], int rows, int cols)
{
    double A[4];
    if (!px2ll || rows < 1 || cols < 1 || !invert2(px2ll, A)) return -1;
    const double lat = px2ll[3] + px2ll[4] * (cols * 0.5) + px2ll[5] * (rows * 0.5);
    if (!(std::fabs(lat) <= kMaxLat)) return -1;
    const double det = std::fabs(px2ll[1] * px2ll[5] - px2ll[2] * px2ll[4]);
    const double s0 = 256.0 / 360.0 * std::sqrt(det / std::cos(lat * kPi / 180.0));          // output pixels per source pixel at z = 0
    for (int z = 0; z <= kMaxZoom; z++)
        if (s0 * (double)(1ll << z) >= 0.70710678118654752440) return z;
    return kMaxZoom;
}

inline const char* plan_message(PlanResult r)
{
    switch (r) {
    case kPlanBadZoom: return "the zoom is outside 0 .. 24";
    case kPlanSingular: return "the 2 x 2 part of the georeference is singular (a vertical plane?)";
    case kPlanLatitude: return "a corner of the image lies beyond 85.05 degrees of latitude";
    case kPlanCapacity: return "the tables need more room than the caller gave";
    case kPlanArguments: return "no georeference, no range or a size that is not positive";
    default: return "ok";
    }
}

}  // namespace webtiles
}  // namespace pf
