// frame_plan.hpp -- the plan of one keyframe: which cells of its canvas can be left out (the cull's bounds), where each pyramid level
// must be computed and which blocks of a launch run.  Host arithmetic on integers and doubles alone (no device, no tile store, no lock,
// no HIP header), so that the product, the CPU tests and the sanitizer program (tests/cpp/frame_plan_check.cpp) compile the very same code.
#pragma once
#include "plan_limits.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pf {

struct Win { int x0, x1, y0, y1; };      // [x0,x1) x [y0,y1)

// ---------------------------------------------------------------------------------------------------------------- cull bounds
// A cell of a tile in which a keyframe cannot win the max-weight select at ANY level is left out of its launch (fusion_map.cpp,
// build_tile_table, has the argument).  Both sides are bounded from the geometry alone, with margins.

// Margins of the bounds (cell_out): source pixels added to / taken from a distance before it becomes a weight (the nearest-pixel
// rounding of the weight gather, 0.71 px, and the float arithmetic of the kernels), and what is taken from / added to a weight (the
// pyramid's own rounding); sub: cells per tile edge (4; experiments library, PF_CULL_SUB=2: quadrants).
struct CullMargins { double px = 2.0, w = 1e-5; int sub = 4; };

// May this frame's tiles be culled?  Only for a tame map: every canvas corner (with the pyramid halo) in front of the camera and
// far inside the int range, as the kernels' fast path assumes -- anything else renders every tile.
inline bool cull_frame_ok(const double M[9], int crows, int ccols)
{
    const double xs[2] = { -600.0, ccols + 600.0 }, ys[2] = { -600.0, crows + 600.0 };
    int sign = 0;
    for (int i = 0; i < 4; i++) {
        const double x = xs[i & 1], y = ys[i >> 1], W = M[6] * x + M[7] * y + M[8];
        if (!(std::fabs(W) > 1e-12) || !std::isfinite(W)) return false;
        const int sg = W > 0 ? 1 : -1;
        if (sign && sg != sign) return false;
        sign = sg;
        if (!(std::fabs((M[0] * x + M[1] * y + M[2]) / W) < 1.0e7) || !(std::fabs((M[3] * x + M[4] * y + M[5]) / W) < 1.0e7)) return false;
    }
    return true;
}

// Map2DCPU (single band): no pyramid, so a cell is not dilated; the bounds are those of the radial weight all the same, compared
// three alpha steps apart -- the stored alpha byte is floor(254 w) (at least 2) interpolated with 15-bit taps (within 1 of its smallest
// tap), the select is `ele.a < dst.a` (Map2DCPU.cpp:326-327): the keyframe cannot win where 254 wmax <= 254 wlb - 3.
// What cell_out compares the keyframe's weights with:
inline float stored_bound(float wlb, bool single_band)
{
    const float gap = single_band ? 3.2f / 254.f : 0.f, floor_w = single_band ? 6.f / 254.f : 0.f;
    return wlb > floor_w ? wlb - gap : 0.f;
}

// what a keyframe does to one tile of its canvas (Lattice::tile_cull)
struct TileCull {
    unsigned out;                       // 64 x 64 cells in which the keyframe cannot win (bit 4 * row + column)
    int nraise; int q[16]; float w[16]; // cells whose lower bound the keyframe raises: wlb[q] -> w, once the frame is in
};

// The Lipschitz constant of a keyframe's map on its canvas: s >= sup ||J_H||_2 over the rectangle [x0, x1] x [y0, y1] of canvas pixels,
// H(x) = (A x + b) / W(x), W(x) = g . x + h.  J = (A - H(x) g^T) / W(x), so ||J|| <= (||A||_2 + |H(x)| |g|) / |W(x)|; W is linear and keeps
// its sign on the rectangle (cull_frame_ok asks for more), |H| is convex on the rectangle's image (a convex quadrilateral): both extrema
// sit at corners.  The exact 2-norm of the 2 x 2 block (its largest singular value), not the Frobenius norm.
inline double map_lipschitz(const double M[9], double x0, double x1, double y0, double y1)
{
    const double t = M[0] * M[0] + M[1] * M[1] + M[3] * M[3] + M[4] * M[4], det = M[0] * M[4] - M[1] * M[3];
    const double nA = std::sqrt(0.5 * (t + std::sqrt(std::max(t * t - 4.0 * det * det, 0.0))));
    const double xs[2] = { x0, x1 }, ys[2] = { y0, y1 };
    double hmax = 0, wmin = 1e300;
    for (int i = 0; i < 4; i++) {
        const double x = xs[i & 1], y = ys[i >> 1], W = M[6] * x + M[7] * y + M[8];
        hmax = std::max(hmax, std::hypot(M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5]) / std::fabs(W));
        wmin = std::min(wmin, std::fabs(W));
    }
    const double s = (nA + hmax * std::hypot(M[6], M[7])) / wmin;
    return std::isfinite(s) ? s : 1e30;
}
// The slack of the pyramid, source pixels: a weight of level i <= L is the level-0 weight image under the i-fold composition of pyrDown's
// [1 4 6 4 1] / 16, centred on the pixel's own level-0 position with variance (4^i - 1) / 3 per axis (BORDER_REFLECT_101 only folds mass
// towards positions inside the canvas), so E |x - 2^i p| <= sqrt(2 (4^L - 1) / 3) level-0 pixels, s times that in the source.
inline double pyramid_slack(double s, int L)
{
    return L <= 0 ? 0.0 : s * std::sqrt(2.0 * (std::ldexp(1.0, 2 * L) - 1.0) / 3.0);
}

// The canvas lattice (64 (k - off), 64 (m - off)), k = 0 .. ccols / 64 + 2 off, mapped into the source frame: position, squared distance
// from the image centre, inside-the-frame flag.  A cell's rectangles have their corners on it: the one the distance extrema are taken
// over (the cell dilated by `dil` lattice steps) and the one that must map inside the frame before a lower bound is given (dilated by
// `idil` steps: the support of the pyramid); off = max(dil, idil).  `slack`: source pixels added to the margin mg.px on both sides
// (pyramid_slack) -- with it the extrema are those of the cell itself (dil 0) and only the inside test keeps the dilation.
struct Lattice {
    bool all = false; int nx = 0, ny = 0, dil = 1, idil = 1, off = 1, cols = 0, rows = 0; double xc = 0, yc = 0, dis_max = 1, inv_dis_max = 1, M[9] = {};
    double slack = 0;
    CullMargins mg;
    std::vector<double> sx, sy, d; std::vector<unsigned char> in;
    std::vector<double> pair_d; std::vector<unsigned char> pair_in; bool paired = false;      // raise_bounds' fast route

    // Points are mapped on first use (a shard asks for an eighth of them) unless map_all; one division per point, no square root.
    // in_dil < 0: the inside test over the same rectangle as the extrema (dil)
    void map_canvas(const double Minv[9], int crows, int ccols, int cols_, int rows_, int dil_, bool map_all, const CullMargins& m, int in_dil = -1,
                    double slack_ = 0.0)
    {
        all = map_all; mg = m; paired = false;
        dil = dil_;                                                 // dilation of a cell in lattice steps of 64 pixels
        idil = in_dil < 0 ? dil_ : in_dil; off = std::max(dil, idil); slack = slack_;
        nx = ccols / 64 + 2 * off + 1; ny = crows / 64 + 2 * off + 1;
        const size_t n = (size_t)nx * ny;
        sx.resize(n); sy.resize(n); d.resize(n); in.assign(n, 2);      // 2: not mapped yet
        xc = (double)(cols_ / 2); yc = (double)(rows_ / 2); dis_max = std::sqrt(xc * xc + yc * yc);
        inv_dis_max = 1.0 / dis_max;
        cols = cols_; rows = rows_;
        for (int i = 0; i < 9; i++) M[i] = Minv[i];
        if (!map_all) return;                                       // a shard that owns a small part of the canvas asks for a fraction of the points: on first use
        // unsharded (or a shard that owns most of this canvas: the replicas of bench.py's weak mode own all of it), every point is needed (a cell's
        // rectangles have their corners on neighbouring points): all of them now, row by row,
        // in loops without branches that the compiler turns into packed divisions (a third of the time of mapping them one by one)
        const double cmax = cols - 2.0, rmax = rows - 2.0;
        for (int m_ = 0; m_ < ny; m_++) {
            const double y = 64.0 * (m_ - off), n0 = M[1] * y + M[2], n1 = M[4] * y + M[5], w0 = M[7] * y + M[8];
            double* __restrict__ psx = sx.data() + (size_t)m_ * nx; double* __restrict__ psy = sy.data() + (size_t)m_ * nx;
            double* __restrict__ pd = d.data() + (size_t)m_ * nx; unsigned char* __restrict__ pin = in.data() + (size_t)m_ * nx;
            for (int k = 0; k < nx; k++) {
                const double x = 64.0 * (k - off), iw = 1.0 / (M[6] * x + w0);
                const double px = (M[0] * x + n0) * iw, py = (M[3] * x + n1) * iw, dx = px - xc, dy = py - yc;
                psx[k] = px; psy[k] = py; pd[k] = dx * dx + dy * dy;
            }
            for (int k = 0; k < nx; k++) pin[k] = (unsigned char)((psx[k] >= 1.0) & (psx[k] <= cmax) & (psy[k] >= 1.0) & (psy[k] <= rmax));
        }
    }

    size_t point(int k, int m)
    {
        const size_t o = (size_t)m * nx + k;
        if (in[o] == 2) {
            const double x = 64.0 * (k - off), y = 64.0 * (m - off), iw = 1.0 / (M[6] * x + M[7] * y + M[8]);
            const double px = (M[0] * x + M[1] * y + M[2]) * iw, py = (M[3] * x + M[4] * y + M[5]) * iw;
            sx[o] = px; sy[o] = py;
            const double dx = px - xc, dy = py - yc;
            d[o] = dx * dx + dy * dy;
            in[o] = px >= 1.0 && px <= cols - 2.0 && py >= 1.0 && py <= rows - 2.0;
        }
        return o;
    }

    // The radial weight (weightImage, MultiBandMap2DCPU.cpp:396-418, gathered at the NEAREST source pixel, 0 outside the frame) over the canvas
    // rectangle 64 (k - dil, m - dil) .. 64 (k + span + dil, m + span + dil) -- the cell (k, m) of the canvas (span lattice steps on a side)
    // dilated by 64 dil pixels -- against `wlb`, the lower bound of what the cell stores:
    //   returns true when every weight the keyframe can have there is below wlb (the cell is out);
    //   *wmin <= every weight it has there (0 unless the rectangle maps wholly inside the frame).
    // The rectangle maps to a convex quadrilateral Q of the source plane (M is projective and W keeps its sign, cull_frame_ok); the weight
    // falls with the distance from the image centre c, so the largest weight sits at the point of Q nearest to c and the smallest at its
    // farthest corner.  "Largest weight < wlb" <=> dist(c, Q) > T, T the distance at which the weight -- with the margins -- reaches
    // wlb; decided from the corners alone when one of them lies within T (most cells that stay in), by the exact point-to-quadrilateral
    // distance otherwise.
    //
    // With a slack (map_canvas) the weights bounded are those of EVERY pyramid level at the pixels whose level-0 position lies in the cell:
    // such a weight is a convex combination of level-0 weights around that position, and differs from the radial weight AT the position by
    // at most slack / dis_max (fusion_map.cpp, build_tile_table, has the argument).  The slack joins the pixel margin on both sides; the
    // upper side bounds the combination through the Lipschitz function max(1 - d / dis_max, floor) >= weight, so a bound at or below
    // floor + slack / dis_max culls nothing (floor: the weight image's own 1e-5, its square root for squared weights); the lower side
    // needs every point of the combination inside the frame: the corners of the cell dilated by idil steps.
    bool cell_out(int k, int m, int span, int weight_type, float wlb, bool want_out, float* wmin)
    {
        const int e = span + 2 * dil, o = off - dil;                   // lattice steps across the dilated cell; its first corner
        const size_t c[4] = { point(k + o, m + o), point(k + o + e, m + o), point(k + o + e, m + o + e), point(k + o, m + o + e) };
        const double d2[4] = { d[c[0]], d[c[1]], d[c[2]], d[c[3]] };
        const double mpx = mg.px + slack, mw = mg.w;
        if (wmin) {                                                    // (nullptr: only the question whether the cell is out)
            *wmin = 0.f;
            // (weight type 0: wmin can exceed wlb only if the farthest corner lies within (1 - 1e-5 - wlb) dis_max - 2 of the centre -- in the steady
            // state it rarely does, and the square root is not taken)
            const double far2 = std::max(std::max(d2[0], d2[1]), std::max(d2[2], d2[3]));
            const double tw = weight_type == 0 ? (1.0 - mw - (double)wlb) * dis_max - mpx : 1e300;
            bool inside = tw > 0 && far2 < tw * tw * (1.0 + 1e-9);
            if (inside) {
                if (idil == dil) inside = (in[c[0]] & in[c[1]] & in[c[2]] & in[c[3]]) == 1;
                else {
                    const int ei = span + 2 * idil, oi = off - idil;
                    inside = (in[point(k + oi, m + oi)] & in[point(k + oi + ei, m + oi)] & in[point(k + oi + ei, m + oi + ei)] & in[point(k + oi, m + oi + ei)]) == 1;
                }
            }
            if (inside) {
                const double dfar = std::sqrt(far2) + mpx;
                double w = 1.0 - dfar * inv_dis_max;
                if (weight_type != 0) w = w > 0 ? w * w : 0.0;
                w -= mw;
                if (w > 2e-5) *wmin = (float)w;
            }
        }
        if (!want_out || !(wlb > 2e-5f)) return false;                // nothing known about the stored weights (or a fresh tile): in
        // T: weight(T - mpx) + mw == wlb
        double g = (double)wlb - mw;
        if (weight_type != 0) g = std::sqrt(g);
        if (slack > 0 && !(g - slack * inv_dis_max > (weight_type != 0 ? 3.1623e-3 : 1e-5))) return false;      // within the slack of the weights' floor
        const double T = mpx + dis_max * (1.0 - g), T2 = T * T;
        if (d2[0] <= T2 || d2[1] <= T2 || d2[2] <= T2 || d2[3] <= T2) return false;      // a corner within T
        bool pos = true, neg = true; double dnear2 = 1e300;
        for (int i = 0; i < 4; i++) {
            const size_t a = c[i], b = c[(i + 1) & 3];
            const double ex = sx[b] - sx[a], ey = sy[b] - sy[a], px = xc - sx[a], py = yc - sy[a];
            const double cr = ex * py - ey * px;
            pos = pos && cr >= 0; neg = neg && cr <= 0;
            const double e2 = ex * ex + ey * ey, dot = px * ex + py * ey;
            // squared distance from c to the segment: the end points are the corners (known to lie beyond T), the foot of the perpendicular counts
            // only when it falls inside the segment
            if (dot > 0 && dot < e2) dnear2 = std::min(dnear2, cr * cr / e2);
        }
        if (pos || neg) return false;                               // the centre lies inside Q: the keyframe's best weights are here
        return dnear2 > T2;
    }

    // The weight bounds of an admitted keyframe go into tile (x, y)'s wlb, which only ever rises.  A keyframe never culls itself by this:
    // the largest weight it can have in a cell is not below the smallest (cell_out's margins only widen the gap).
    void raise_bounds(int x, int y, int weight_type, float wlb[16])
    {
        if (all && mg.sub == 4) raise_bounds_fast(x, y, weight_type, wlb); else raise_bounds_cells(x, y, weight_type, wlb);
    }
    // the general route: cell by cell through cell_out
    void raise_bounds_cells(int x, int y, int weight_type, float wlb[16])
    {
        const int S = mg.sub, span = 4 / S;
        for (int q = 0; q < S * S; q++) {
            float wmin;
            (void)cell_out(4 * x + span * (q % S), 4 * y + span * (q / S), span, weight_type, wlb[q], false, &wmin);
            if (wmin > 0.f && wmin > wlb[q]) wlb[q] = wmin;          // (wmin 0: nothing known -- a bound of -1 stays, as on the fast route)
        }
    }
    // Every lattice point is mapped (map_canvas), 4 x 4 cells: the same arithmetic as cell_out's first half, without its calls -- the farthest
    // corner of a cell's dilated square from a pass (once per keyframe) that pairs the points e steps apart along a row first -- two pairings:
    // the distances e = 1 + 2 dil apart, the inside flags ei = 1 + 2 idil apart.  For host time.
    void raise_bounds_fast(int x, int y, int weight_type, float wlb[16])
    {
        const int e = 1 + 2 * dil, o = off - dil, ei = 1 + 2 * idil, oi = off - idil;
        if (!paired) {
            pair_d.resize((size_t)nx * ny); pair_in.resize((size_t)nx * ny);
            for (int m = 0; m < ny; m++) {
                const double* __restrict__ dd = d.data() + (size_t)m * nx; const unsigned char* __restrict__ ii = in.data() + (size_t)m * nx;
                double* __restrict__ pd = pair_d.data() + (size_t)m * nx; unsigned char* __restrict__ pi = pair_in.data() + (size_t)m * nx;
                for (int k = 0; k + e < nx; k++) pd[k] = std::max(dd[k], dd[k + e]);
                for (int k = 0; k + ei < nx; k++) pi[k] = ii[k] & ii[k + ei];
            }
            paired = true;
        }
        const double mpx = mg.px + slack, mw = mg.w;
        for (int qy = 0; qy < 4; qy++) {
            const size_t r0 = (size_t)(4 * y + qy + o) * nx + 4 * x + o, r1 = r0 + (size_t)e * nx;
            const size_t i0 = (size_t)(4 * y + qy + oi) * nx + 4 * x + oi, i1 = i0 + (size_t)ei * nx;
            for (int qx = 0; qx < 4; qx++) {
                if (!(pair_in[i0 + qx] & pair_in[i1 + qx])) continue;              // not wholly inside the frame: wmin 0
                float& wl = wlb[4 * qy + qx];
                const double far2 = std::max(pair_d[r0 + qx], pair_d[r1 + qx]);
                const double tw = weight_type == 0 ? (1.0 - mw - (double)wl) * dis_max - mpx : 1e300;
                if (!(tw > 0 && far2 < tw * tw * (1.0 + 1e-9))) continue;
                const double dfar = std::sqrt(far2) + mpx;
                double ww = 1.0 - dfar * inv_dis_max;
                if (weight_type != 0) ww = ww > 0 ? ww * ww : 0.0;
                ww -= mw;
                if (ww > 2e-5 && (float)ww > wl) wl = (float)ww;
            }
        }
    }

    // The decision for tile (x, y) of the canvas, whose cells store weights of at least wlb[].
    // The whole tile first, against the smallest of its cells' bounds: out there is out in every cell (the tile's dilated rectangle holds
    // each cell's) -- most culled cells lie in such tiles; without lookahead their wmin is still worked out cell by cell, with it the
    // bounds went into wlb when the keyframe was admitted (pre_raised) and the cells are skipped.
    // A FRESH tile (no keyframe has written it: its first one copies unconditionally, MultiBandMap2DCPU.cpp:498) is rendered whole or not
    // at all: its slot holds no weights a select could be run against, so no single cell may be left out.  It can be left out whole only
    // through the lookahead -- its wlb then holds bounds of keyframes that wait behind this one; the one whose bound is the largest in a
    // cell is never out there and renders the tile (all of it) before anybody looks.  Without lookahead a fresh tile's wlb is -1 and
    // nothing is out.
    void tile_cull(int x, int y, const float wlb[16], bool fresh, bool lookahead, bool pre_raised, int weight_type, bool single_band, TileCull& c)
    {
        const int S = mg.sub, span = 4 / S;
        c.out = 0; c.nraise = 0;
        bool tile_out = false;
        const bool ask = !fresh || lookahead;
        if (ask) {
            float wl = wlb[0];
            for (int q = 1; q < S * S; q++) wl = std::min(wl, wlb[q]);
            tile_out = cell_out(4 * x, 4 * y, 4, weight_type, stored_bound(wl, single_band), true, nullptr);
        }
        if (tile_out && pre_raised) c.out = 0xffffu;       // (the keyframe's own bounds are in wlb since it was admitted)
        else for (int q = 0; q < S * S; q++) {
            const int qx = q % S, qy = q / S;
            float wmin = 0.f;
            if (cell_out(4 * x + span * qx, 4 * y + span * qy, span, weight_type, stored_bound(wlb[q], single_band), ask && !tile_out, pre_raised ? nullptr : &wmin) || tile_out)
                c.out |= S == 4 ? 1u << q : 0x33u << (8 * qy + 2 * qx);
            if (wmin > wlb[q]) { c.q[c.nraise] = q; c.w[c.nraise++] = wmin; }
        }
        if (fresh && c.out != 0xffffu) c.out = 0;
    }
};

// ----------------------------------------------------------------------------------------------------------------- level plan
inline void clampw(int lo, int hi, int n, int& o0, int& o1) { o0 = std::max(lo, 0); o1 = std::min(hi, n); }
// a box of level-0 pixels (multiples of 64) at level i: floor / ceil (at the top levels a cell is less than a pixel)
inline int lv_lo(int p, int i) { return p >> i; }
inline int lv_hi(int p, int i) { return (p + (1 << i) - 1) >> i; }

// Where Gaussian level i must be valid so that the Laplacian of what is rendered inside `box` (level-0 pixels) is exact (pixel-exact:
// pyrDown reads [2p-2, 2p+2], pyrUp +-1), clamped to the canvas
inline void need_windows(const Win& box, int L, int crows, int ccols, Win N[kMaxLevels])
{
    for (int i = L; i >= 0; i--) {
        int x0 = lv_lo(box.x0, i), x1 = lv_hi(box.x1, i), y0 = lv_lo(box.y0, i), y1 = lv_hi(box.y1, i);
        if (i > 0) { x0 -= 1; x1 += 1; y0 -= 1; y1 += 1; }
        if (i < L) {
            x0 = std::min(x0, 2 * N[i + 1].x0 - 2); x1 = std::max(x1, 2 * N[i + 1].x1 + 1);
            y0 = std::min(y0, 2 * N[i + 1].y0 - 2); y1 = std::max(y1, 2 * N[i + 1].y1 + 1);
        }
        clampw(x0, x1, ccols >> i, N[i].x0, N[i].x1);
        clampw(y0, y1, crows >> i, N[i].y0, N[i].y1);
    }
}

typedef unsigned __int128 u128;
// bits x0 .. x1 of a 128-bit row of cells
inline u128 col_mask(int x0, int x1) { return (x1 - x0 >= 127 ? ~(u128)0 : (((u128)1 << (x1 - x0 + 1)) - 1)) << x0; }

// the hash cells (of a shard; for the cull alone squares of tiles) something is rendered in, each with the box of that, level-0 pixels
struct CellList {
    struct Cell { int cx, cy, x0, y0, x1, y1; };
    Cell c[64]; int n = 0; bool overflow = false;         // more than 64 cells: overflow, and every block runs
    void add(int cx, int cy, int x0, int y0, int x1, int y1)
    {
        if (overflow) return;
        int k = n - 1;
        while (k >= 0 && !(c[k].cx == cx && c[k].cy == cy)) k--;
        if (k < 0) {
            if (n == 64) overflow = true;
            else c[n++] = Cell{ cx, cy, x0, y0, x1, y1 };
        } else {
            Cell& e = c[k];
            e.x0 = std::min(e.x0, x0); e.y0 = std::min(e.y0, y0); e.x1 = std::max(e.x1, x1); e.y1 = std::max(e.y1, y1);
        }
    }
};

// Fused forms: where the level kernels run.
//   need[i]      Gaussian level i must be valid here so that the Laplacian of the rendered box is exact
//   C[i]         compute region of level i: its launch must cover the owned tiles and produce GW_{i+1} wherever the level i+1
//                launch stages its halo (its region -4 / +3)
//   need bitmaps upper levels: one bit per block of the level's grid -- does a rendered cell lie within the pyramid's reach of it (the
//                rule the level-0 blocks apply to themselves in the kernel: (3 * 2^(L-i) - 2) level-i pixels)?  From row bitmaps of the
//                rendered cells (canvases up to 32 tiles wide); the jobs carry them in their launches' kernel arguments
//   rectangles   a shard's tiles are scattered hash cells, and the compute regions are their bounding box: per level, one rectangle of
//                64 x BH blocks per cell says where something owned depends on a block (the same recursion as `need`, applied per
//                cell); blocks outside every rectangle exit at once.  The fallback of the bitmaps.  (Unsharded, no cull: every block runs.)
struct LevelPlan {
    Win need[kMaxLevels], C[kMaxLevels];
    BlockRect rects[kMaxLevels][kMaxRects]; int nrect[kMaxLevels], need_n[kMaxLevels];
    uint32_t need_bits[kMaxLevels][kNeedWords];     // the upper levels' need bitmaps (need_n[i] blocks; 0: none)
    double blocks_run0;                             // level-0 blocks that run
    bool partial;                                   // the cull or a shard leaves blocks out
    bool merged;                                    // some level had more rectangles than its job carries: pairs were merged (diagnostics)
    int L, tx, ty, BH, reach0;
    // scratch, kept between keyframes for its capacity
    std::vector<u128> cell_rows, colmask;           // rendered cells of the canvas, one 128-bit row per cell row; exact_level0_blocks' column masks
    std::vector<uint8_t> block_bits;
    struct R { int x0, y0, x1, y1; };
    std::vector<R> lv[kMaxLevels];

    void reset() { blocks_run0 = 0; partial = false; merged = false; for (int i = 0; i < kMaxLevels; i++) { nrect[i] = 0; need_n[i] = 0; } }
    int grid_x(int i) const { return (C[i].x1 - C[i].x0 + 63) / 64; }
    int grid_y(int i) const { return (C[i].y1 - C[i].y0 + BH - 1) / BH; }
    int need_count(int i) const { int n = 0; for (int k = 0; k < (need_n[i] + 31) / 32; k++) n += __builtin_popcount(need_bits[i][k]); return n; }

    // need[]: per-level windows of the whole rendered box; level 0 is produced by the warp in 64 x 4 blocks
    void windows(const Win& box, int L_, int crows, int ccols)
    {
        need_windows(box, L_, crows, ccols, need);
        need[0].x0 = (need[0].x0 / 64) * 64; need[0].x1 = std::min(ccols, ((need[0].x1 + 63) / 64) * 64);
        need[0].y0 = (need[0].y0 / 4) * 4;   need[0].y1 = std::min(crows, ((need[0].y1 + 3) / 4) * 4);
    }

    // blocks of level i's grid inside the union of its rectangles
    long count_union(int i)
    {
        const int nbx = grid_x(i), nby = grid_y(i);
        if (nbx <= 0 || nby <= 0) return 0;
        block_bits.assign((size_t)nbx * nby, 0);
        for (int k = 0; k < nrect[i]; k++) {
            const int x0 = std::max<int>(rects[i][k].x0, 0), x1 = std::min<int>(rects[i][k].x1, nbx);
            if (x1 <= x0) continue;
            for (int gy = std::max<int>(rects[i][k].y0, 0); gy < std::min<int>(rects[i][k].y1, nby); gy++) std::memset(block_bits.data() + (size_t)gy * nbx + x0, 1, (size_t)(x1 - x0));
        }
        long n = 0;
        for (uint8_t v : block_bits) n += v;
        return n;
    }

    // table: the canvas' tx x ty entries, 0 = not rendered by this rank, else bits 48.. = the cells that are out; box: around the cells that
    // are rendered, level-0 pixels; BH_: block height of the level kernel; reach0: reach of the level-0 blocks' own need test when their job
    // carries rectangles (0: it takes the rectangles).  Returns whether the rectangles were made (partial, fused == 1).
    bool plan(const uint64_t* table, int tx_, int ty_, int L_, const Win& box, const CellList& cells, bool sharded, bool culled_any, int fused, int BH_, int reach0_)
    {
        L = L_; tx = tx_; ty = ty_; BH = BH_; reach0 = reach0_;
        merged = false;
        const int crows = ty * kElePixels, ccols = tx * kElePixels;
        for (int i = L - 1; i >= 0; i--) {
            // the origin stays even (a block's quads and its part of level i+1 start on even pixels): a box of 64-pixel cells is odd at level 6
            int x0 = lv_lo(box.x0, i) & ~1, x1 = lv_hi(box.x1, i), y0 = lv_lo(box.y0, i) & ~1, y1 = lv_hi(box.y1, i);
            if (i < L - 1) {
                x0 = std::min(x0, 2 * (C[i + 1].x0 - 4)); x1 = std::max(x1, 2 * (C[i + 1].x1 + 3));
                y0 = std::min(y0, 2 * (C[i + 1].y0 - 4)); y1 = std::max(y1, 2 * (C[i + 1].y1 + 3));
            }
            clampw(x0, x1, ccols >> i, C[i].x0, C[i].x1);
            clampw(y0, y1, crows >> i, C[i].y0, C[i].y1);
        }
        partial = (sharded || culled_any) && !cells.overflow;
        if (partial && 4 * tx <= 128 && L >= 2) {
            cell_rows.assign((size_t)4 * ty, 0);
            for (int y = 0; y < ty; y++)
                for (int x = 0; x < tx; x++) {
                    const uint64_t e = table[(size_t)y * tx + x];
                    if (!e) continue;
                    const unsigned in = ~(unsigned)(e >> 48) & 0xffffu;
                    for (int r = 0; r < 4; r++) cell_rows[(size_t)4 * y + r] |= (u128)((in >> (4 * r)) & 15u) << (4 * x);
                }
            for (int i = 1; i < L; i++) {
                const int reach = ((3 << (L - i)) - 2) << i, nbx = grid_x(i), nby = grid_y(i);
                need_n[i] = 0;
                if (nbx <= 0 || nby <= 0 || (nbx * nby + 31) / 32 > kNeedWords) continue;
                uint32_t* bits = need_bits[i];
                std::memset(bits, 0, sizeof(uint32_t) * (size_t)((nbx * nby + 31) / 32));
                for (int gy = 0; gy < nby; gy++) {
                    const int y0 = std::max(((C[i].y0 + gy * BH) << i) - reach, 0) >> 6, y1 = std::min((((C[i].y0 + gy * BH + BH) << i) - 1 + reach) >> 6, 4 * ty - 1);
                    u128 rowsum = 0;
                    for (int r = y0; r <= y1; r++) rowsum |= cell_rows[(size_t)r];
                    if (!rowsum) continue;
                    for (int gx = 0; gx < nbx; gx++) {
                        const int x0 = std::max(((C[i].x0 + gx * 64) << i) - reach, 0) >> 6, x1 = std::min((((C[i].x0 + gx * 64 + 64) << i) - 1 + reach) >> 6, 4 * tx - 1);
                        if (x0 > x1) continue;
                        if (rowsum & col_mask(x0, x1)) { const int b = gy * nbx + gx; bits[(size_t)b >> 5] |= 1u << (b & 31); }
                    }
                }
                need_n[i] = nbx * nby;
            }
        }
        if (!(partial && fused == 1)) return false;
        for (int i = 0; i < L; i++) lv[i].clear();
        for (int c = 0; c < cells.n; c++) {
            // N[i]: where Gaussian level i is needed for this cell's tiles.  The level-i block at b runs iff it holds owned pixels or its
            // part of level i+1 lies in N[i+1]; what else it computes from unproduced input is never read.
            const CellList::Cell& ce = cells.c[c];
            Win N[kMaxLevels];
            need_windows(Win{ ce.x0, ce.x1, ce.y0, ce.y1 }, L, crows, ccols, N);
            for (int i = 0; i < L; i++) {
                int x0 = std::min(lv_lo(ce.x0, i), 2 * N[i + 1].x0), x1 = std::max(lv_hi(ce.x1, i), 2 * N[i + 1].x1);
                int y0 = std::min(lv_lo(ce.y0, i), 2 * N[i + 1].y0), y1 = std::max(lv_hi(ce.y1, i), 2 * N[i + 1].y1);
                x0 = std::max(x0, C[i].x0); y0 = std::max(y0, C[i].y0); x1 = std::min(x1, C[i].x1); y1 = std::min(y1, C[i].y1);
                if (x0 >= x1 || y0 >= y1) continue;
                lv[i].push_back(R{ (x0 - C[i].x0) / 64, (y0 - C[i].y0) / BH, (x1 - C[i].x0 + 63) / 64, (y1 - C[i].y0 + BH - 1) / BH });
            }
        }
        for (int i = 0; i < L; i++) {
            // at most kMaxRects (level 0) / kMaxRectsUpper travel with a job: merge the pair whose common bounding box adds the fewest blocks
            // (extra blocks only cost time: they hold no owned pixel and write no tile)
            std::vector<R>& v = lv[i];
            auto area = [](const R& r) { return (long)(r.x1 - r.x0) * (r.y1 - r.y0); };
            const int cap = i == 0 ? kMaxRects : kMaxRectsUpper;       // what a job of this level can carry (plan_limits.hpp)
            if ((int)v.size() > cap) merged = true;
            while ((int)v.size() > cap) {
                size_t ba = 0, bb = 1; long best = -1;
                for (size_t p = 0; p < v.size(); p++)
                    for (size_t q = p + 1; q < v.size(); q++) {
                        const R u{ std::min(v[p].x0, v[q].x0), std::min(v[p].y0, v[q].y0), std::max(v[p].x1, v[q].x1), std::max(v[p].y1, v[q].y1) };
                        const long add = area(u) - area(v[p]) - area(v[q]);
                        if (best < 0 || add < best) { best = add; ba = p; bb = q; }
                    }
                v[ba] = R{ std::min(v[ba].x0, v[bb].x0), std::min(v[ba].y0, v[bb].y0), std::max(v[ba].x1, v[bb].x1), std::max(v[ba].y1, v[bb].y1) };
                v.erase(v.begin() + bb);
            }
            nrect[i] = (int)v.size();
            for (int k = 0; k < nrect[i]; k++) rects[i][k] = BlockRect{ (short)v[k].x0, (short)v[k].y0, (short)v[k].x1, (short)v[k].y1 };
            if (v.empty()) { nrect[i] = 1; rects[i][0] = BlockRect{ 0, 0, 0, 0 }; }      // nothing needed at this level: an empty rectangle
        }
        // level-0 blocks that run (render_stats, bench --shard strong; the numerator of roofline.frac)
        if (need_n[1] > 0 && reach0 > 0)
            // the level-0 blocks pick themselves in the kernel (within 94 px of a rendered cell): counted through the level-1 bitmap, whose
            // blocks are 2 x 2 of them under nearly the same rule (92 px)
            blocks_run0 = std::min(4.0 * need_count(1), (double)grid_x(0) * grid_y(0));
        else blocks_run0 = (double)count_union(0);
        return true;
    }

    // Accounting of a pipelined launch: share of each level's canvas pixels (owned_all tiles of this rank) that the blocks which RUN cover:
    // 1 unless the cull or a shard leaves blocks out.  Level 0 with the blocks' own need test (k_levels, need_r0): through the level-1
    // bitmap here, and -- when the launch is bracketed by events (exact_wanted) -- exactly, after the launch is out (exact_level0_share):
    // *exact_r0 is then the reach to call it with.
    void run_shares(int owned_all, bool exact_wanted, double run_share[kMaxLevels], int* exact_r0)
    {
        *exact_r0 = 0;
        for (int i = 0; i < kMaxLevels; i++) run_share[i] = 1.0;
        if (!partial) return;
        for (int i = 0; i < L; i++) {
            const int nbx = grid_x(i), nby = grid_y(i);
            if (nbx <= 0 || nby <= 0) continue;
            double run;
            if (i == 0) {
                run = blocks_run0;
                // counted exactly AFTER the launch is out: ~50 us of host time that must not delay it
                if (need_n[1] > 0 && reach0 > 0 && exact_wanted && cell_rows.size() == (size_t)4 * ty) *exact_r0 = reach0;
            } else if (need_n[i] > 0) run = need_count(i);
            else run = nrect[i] ? (double)count_union(i) : (double)nbx * nby;
            const double ts = kElePixels >> i;
            run_share[i] = std::min(1.0, run * 64.0 * BH / std::max(1.0, (double)owned_all * ts * ts));
        }
    }

    // the blocks' own need rule (k_levels need_r0) evaluated from the rendered cells' row bitmaps: the level-0 blocks that run
    // (the column masks once per launch, one AND per block: ~8 us for cfg-A's 7072 blocks)
    long exact_level0_blocks(int r0)
    {
        const int nbx = grid_x(0), nby = grid_y(0), crows = ty * kElePixels, ccols = tx * kElePixels;
        colmask.assign((size_t)std::max(nbx, 0), 0);
        for (int gx = 0; gx < nbx; gx++) {
            const int x0 = std::max(C[0].x0 + gx * 64 - r0, 0) >> 6, x1 = std::min(C[0].x0 + gx * 64 + 63 + r0, ccols - 1) >> 6;
            if (x0 <= x1) colmask[(size_t)gx] = col_mask(x0, x1);
        }
        long run = 0;
        for (int gy = 0; gy < nby; gy++) {
            const int y0 = std::max(C[0].y0 + gy * BH - r0, 0) >> 6, y1 = std::min(C[0].y0 + gy * BH + BH - 1 + r0, crows - 1) >> 6;
            u128 rowsum = 0;
            for (int r = y0; r <= y1; r++) rowsum |= cell_rows[(size_t)r];
            if (!rowsum) continue;
            const uint64_t lo = (uint64_t)rowsum, hi = (uint64_t)(rowsum >> 64);
            for (int gx = 0; gx < nbx; gx++) run += ((lo & (uint64_t)colmask[(size_t)gx]) | (hi & (uint64_t)(colmask[(size_t)gx] >> 64))) != 0;
        }
        return run;
    }
    // ... as the share of the level-0 canvas pixels that they cover
    double exact_level0_share(int owned_all, int r0)
    {
        return std::min(1.0, exact_level0_blocks(r0) * 64.0 * BH / std::max(1.0, (double)owned_all * kElePixels * kElePixels));
    }
};

}  // namespace pf
