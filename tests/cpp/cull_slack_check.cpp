// The cull's bounds with the pyramid's slack (frame_plan.hpp: Lattice with dil 0, an inside test over the pyramid's reach and
// pyramid_slack(map_lipschitz(...), L)) against the weights themselves, on the host, under ASan + UBSan (tests/test_cull_slack.py).
//
// For seeded random tame homographies (a pinhole camera over the ground plane: yaw over the full circle, tilt up to the 0.4 down-look gate
// of footprint(), 0.5 - 4 canvas pixels per source pixel, frames of 320 x 240 to 640 x 480, canvases of 1 - 4 tiles a side) the keyframe's
// weight image is computed on its canvas by the reference's rule (the radial weight at the NEAREST source pixel, 0 outside the frame) and
// reduced with pyrDown in fp32 ([1 4 6 4 1] / 16 per axis, BORDER_REFLECT_101) down to level 8.  For L = 0, 1, 4, 6, 8 and both weight
// types, every cell and every pixel p of a level i <= L whose level-0 position (p << i) lies in the cell:
//   (a) the cell is NOT out against a stored bound equal to the largest such weight   (W_i(p) <= ub)
//   (b) the lower bound the cell gives, where it gives one, is <= the smallest such weight
//   (c) the same for whole tiles (tile_cull's first test)
//   (d) both routes of raise_bounds give the same bits under the new rule
// and, so that none of it passes vacuously: the share of cells with a lower bound, the cells the new rule culls against given bounds
// that the dilated rule leaves in, and a control -- with the slack forced to 0 at L >= 4 the lower bound IS violated somewhere.
#include "frame_plan.hpp"
#include <cstdio>
#include <cstdlib>

using namespace pf;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("VIOLATION: " __VA_ARGS__); std::printf("\n"); if (++g_fail > 20) { std::printf("too many\n"); std::exit(1); } } } while (0)

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_seed >> 33); }
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

static void mul3(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += A[3 * i + k] * B[3 * k + j]; C[3 * i + j] = s; }
}

// MultiBandMap2DCPU.cpp:396-418 at the nearest pixel
static float radial_weight(double sx, double sy, int cols, int rows, int weight_type)
{
    const long j = std::lround(sx), i = std::lround(sy);
    if (j < 0 || i < 0 || j >= cols || i >= rows) return 0.f;
    const double xc = cols / 2, yc = rows / 2, dmax = std::sqrt(xc * xc + yc * yc);
    double w = 1 - std::sqrt((i - yc) * (i - yc) + (j - xc) * (j - xc)) / dmax;
    if (weight_type != 0) w = w * w;
    return (float)(w <= 1e-5 ? 1e-5 : w);
}

static int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// pyrDown, fp32, rows then columns, (n + 1) / 2 outputs per axis
static void pyr_down(const std::vector<float>& src, int rows, int cols, std::vector<float>& dst, int& orows, int& ocols)
{
    orows = (rows + 1) / 2; ocols = (cols + 1) / 2;
    std::vector<float> tmp((size_t)rows * ocols);
    for (int y = 0; y < rows; y++) {
        const float* s = src.data() + (size_t)y * cols;
        for (int x = 0; x < ocols; x++) {
            const float a = s[reflect101(2 * x - 2, cols)], b = s[reflect101(2 * x - 1, cols)], c = s[reflect101(2 * x, cols)], d = s[reflect101(2 * x + 1, cols)],
                        e = s[reflect101(2 * x + 2, cols)];
            tmp[(size_t)y * ocols + x] = c * 6.f + (b + d) * 4.f + a + e;
        }
    }
    dst.assign((size_t)orows * ocols, 0.f);
    for (int y = 0; y < orows; y++) {
        const float* r[5];
        for (int k = 0; k < 5; k++) r[k] = tmp.data() + (size_t)reflect101(2 * y - 2 + k, rows) * ocols;
        for (int x = 0; x < ocols; x++) dst[(size_t)y * ocols + x] = (r[2][x] * 6.f + (r[1][x] + r[3][x]) * 4.f + r[0][x] + r[4][x]) * (1.f / 256.f);
    }
}

static long n_samples, n_rejected, n_cells, n_lb_pos, n_ub_checked, n_out_at_wmax, n_tiles, n_new_only, n_old_only, n_both_out, n_control_viol, n_control_cells,
            n_raise_tiles, n_pixels, n_floor_in;

int main()
{
    const int Ls[5] = { 0, 1, 4, 6, 8 };
    const float bounds[6] = { 0.004f, 0.03f, 0.2f, 0.4f, 0.6f, 0.8f };
    const int kSamples = 36;
    while (n_samples < kSamples) {
        const int cols = 320 + 2 * (int)(rnd() % 161), rows = 240 + 2 * (int)(rnd() % 121), tx = 1 + (int)(rnd() % 4), ty = 1 + (int)(rnd() % 4);
        const int crows = ty * 256, ccols = tx * 256;
        const double f = cols * uni(0.7, 1.3), yaw = uni(0, 6.283185307179586), phi = uni(0, 6.283185307179586), sc = uni(0.5, 4.0), h = 100.0;
        // a third of the samples look straight down, the others tilt up to what the gate lets through
        double theta = n_samples % 3 == 0 ? 0.0 : uni(0.02, 1.1);
        double R[9];
        for (;; theta *= 0.85) {
            const double ax = std::cos(phi), ay = std::sin(phi), c = std::cos(theta), s = std::sin(theta), t = 1 - c;
            const double T[9] = { t * ax * ax + c, t * ax * ay, s * ay, t * ax * ay, t * ay * ay + c, -s * ax, -s * ay, s * ax, c };      // Rodrigues, axis (ax, ay, 0)
            const double Z[9] = { std::cos(yaw), -std::sin(yaw), 0, std::sin(yaw), std::cos(yaw), 0, 0, 0, 1 }, F[9] = { 1, 0, 0, 0, -1, 0, 0, 0, -1 };
            double ZT[9];
            mul3(Z, T, ZT); mul3(ZT, F, R);
            bool ok = true;
            for (int i = 0; i < 4; i++) {
                const double u = ((i & 1) ? cols : 0) - cols / 2, v = ((i >> 1) ? rows : 0) - rows / 2;
                ok = ok && -(R[6] * u / f + R[7] * v / f + R[8]) >= 0.4;
            }
            if (ok) break;
        }
        const double lp = h / (f * sc);
        // where the optical axis meets the ground, put at a random place on or near the canvas
        const double gcx = -h * R[2] / R[8], gcy = -h * R[5] / R[8];
        const double gx0 = gcx - uni(-0.2, 1.2) * ccols * lp, gy0 = gcy - uni(-0.2, 1.2) * crows * lp;
        const double K[9] = { f, 0, (double)(cols / 2), 0, f, (double)(rows / 2), 0, 0, 1 }, RT[9] = { R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8] };
        const double G[9] = { lp, 0, gx0, 0, lp, gy0, 0, 0, -h };
        double KR[9], M[9];
        mul3(K, RT, KR); mul3(KR, G, M);
        if (!cull_frame_ok(M, crows, ccols)) { n_rejected++; continue; }
        n_samples++;
        for (int wt = 0; wt < 2; wt++) {
            // the pyramid of the weights, levels 0 .. 8
            std::vector<float> lv[9]; int lr[9], lc[9];
            lr[0] = crows; lc[0] = ccols; lv[0].resize((size_t)crows * ccols);
            for (int y = 0; y < crows; y++)
                for (int x = 0; x < ccols; x++) {
                    const double W = M[6] * x + M[7] * y + M[8];
                    lv[0][(size_t)y * ccols + x] = radial_weight((M[0] * x + M[1] * y + M[2]) / W, (M[3] * x + M[4] * y + M[5]) / W, cols, rows, wt);
                }
            for (int i = 1; i <= 8; i++) pyr_down(lv[i - 1], lr[i - 1], lc[i - 1], lv[i], lr[i], lc[i]);
            const int ncx = 4 * tx, ncy = 4 * ty;
            std::vector<float> wmax((size_t)ncx * ncy, -1.f), wmin((size_t)ncx * ncy, 2.f);
            int done = -1;
            for (int L : Ls) {
                for (int i = done + 1; i <= L; i++)
                    for (int y = 0; y < lr[i]; y++)
                        for (int x = 0; x < lc[i]; x++) {
                            const size_t c = (size_t)((y << i) >> 6) * ncx + ((x << i) >> 6);
                            const float w = lv[i][(size_t)y * lc[i] + x];
                            wmax[c] = std::max(wmax[c], w); wmin[c] = std::min(wmin[c], w); n_pixels++;
                        }
                done = L;
                const int reach = ((2 << L) - 2 + 63) / 64;
                const double far = 64.0 * reach, s = map_lipschitz(M, -far, ccols + far, -far, crows + far), S = pyramid_slack(s, L);
                Lattice lat, part, old, ctl;
                lat.map_canvas(M, crows, ccols, cols, rows, 0, true, CullMargins(), reach, S);
                part.map_canvas(M, crows, ccols, cols, rows, 0, false, CullMargins(), reach, S);
                old.map_canvas(M, crows, ccols, cols, rows, reach, true, CullMargins());              // the dilated rule
                ctl.map_canvas(M, crows, ccols, cols, rows, 0, true, CullMargins(), reach, 0.0);      // control: no slack
                for (int m = 0; m < ncy; m++)
                    for (int k = 0; k < ncx; k++) {
                        const float hi = wmax[(size_t)m * ncx + k], lo = wmin[(size_t)m * ncx + k];
                        float lb = -5.f, lb2 = -5.f, lbo = -5.f, lbc = -5.f;
                        // (a) against a stored weight equal to its own largest the keyframe still wins (srcW >= dstW): the cell must be in
                        const bool out = lat.cell_out(k, m, 1, wt, hi, true, &lb);
                        CHECK(!out, "cell (%d, %d) L %d type %d sample %ld is out against its own largest weight %.9g (S %.3f s %.4f)", k, m, L, wt, n_samples, hi, S, s);
                        CHECK(out == part.cell_out(k, m, 1, wt, hi, true, &lb2) && lb == lb2, "lattice mapped at once and on first use differ at (%d, %d)", k, m);
                        n_ub_checked++;
                        // (b)
                        (void)lat.cell_out(k, m, 1, wt, -1.f, false, &lb);
                        CHECK(lb >= 0.f && (lb == 0.f || lb <= lo), "cell (%d, %d) L %d type %d sample %ld: lower bound %.9g above its smallest weight %.9g (S %.3f s %.4f)", k, m, L, wt,
                              n_samples, lb, lo, S, s);
                        n_cells++; n_lb_pos += lb > 0.f;
                        // the dilated rule is sound too, and a bound of the new rule is never below it by more than the slack costs
                        (void)old.cell_out(k, m, 1, wt, -1.f, false, &lbo);
                        CHECK(lbo == 0.f || lbo <= lo, "dilated rule: lower bound %.9g above %.9g at (%d, %d) L %d", lbo, lo, k, m, L);
                        // the control: the same bounds without the slack
                        if (L >= 4) {
                            (void)ctl.cell_out(k, m, 1, wt, -1.f, false, &lbc);
                            n_control_cells++; n_control_viol += lbc > 0.f && lbc > lo;
                        }
                        // what the new rule culls against given bounds and the dilated one does not, and the other way round
                        for (float b : bounds) {
                            const bool on = lat.cell_out(k, m, 1, wt, b, true, nullptr), oo = old.cell_out(k, m, 1, wt, b, true, nullptr);
                            if (on) CHECK(hi < b, "cell (%d, %d) L %d type %d is out against %g and has weight %.9g", k, m, L, wt, b, hi);
                            n_new_only += on && !oo; n_old_only += oo && !on; n_both_out += on && oo;
                            n_out_at_wmax += on;
                            // a bound within the slack of the weights' floor culls nothing
                            if (!on && oo && S > 0 && std::sqrt((double)b) < 3.2e-3 + S * lat.inv_dis_max) n_floor_in++;
                        }
                    }
                // (c) whole tiles, (d) both routes of raise_bounds
                for (int y = 0; y < ty; y++)
                    for (int x = 0; x < tx; x++) {
                        float hi = -1.f, lo = 2.f;
                        for (int q = 0; q < 16; q++) { hi = std::max(hi, wmax[(size_t)(4 * y + q / 4) * ncx + 4 * x + q % 4]); lo = std::min(lo, wmin[(size_t)(4 * y + q / 4) * ncx + 4 * x + q % 4]); }
                        float lb;
                        CHECK(!lat.cell_out(4 * x, 4 * y, 4, wt, hi, true, &lb), "tile (%d, %d) L %d type %d is out against its own largest weight %.9g", x, y, L, wt, hi);
                        CHECK(lb == 0.f || lb <= lo, "tile (%d, %d) L %d type %d: lower bound %.9g above %.9g", x, y, L, wt, lb, lo);
                        n_tiles++;
                        for (int start = 0; start < 2; start++) {
                            float a[16], b[16], c2[16];
                            for (int q = 0; q < 16; q++) a[q] = b[q] = c2[q] = start ? bounds[rnd() % 6] : -1.f;
                            lat.raise_bounds_fast(x, y, wt, a); lat.raise_bounds_cells(x, y, wt, b); part.raise_bounds(x, y, wt, c2);
                            CHECK(std::memcmp(a, b, sizeof a) == 0 && std::memcmp(a, c2, sizeof a) == 0, "raise_bounds: the routes differ in tile (%d, %d) L %d type %d", x, y, L, wt);
                            for (int q = 0; q < 16; q++)
                                if (!start && a[q] > 0.f) CHECK(a[q] <= wmin[(size_t)(4 * y + q / 4) * ncx + 4 * x + q % 4], "raised bound %g above the cell's smallest weight", a[q]);
                            n_raise_tiles++;
                        }
                        // tile_cull against the cells' own answers
                        float wl[16]; for (int q = 0; q < 16; q++) wl[q] = bounds[rnd() % 6];
                        TileCull tc;
                        lat.tile_cull(x, y, wl, false, true, true, wt, false, tc);
                        for (int q = 0; q < 16; q++)
                            if (tc.out >> q & 1) CHECK(wmax[(size_t)(4 * y + q / 4) * ncx + 4 * x + q % 4] < wl[q], "tile_cull: cell %d of tile (%d, %d) out against %g", q, x, y, wl[q]);
                    }
            }
        }
    }
    std::printf("slack: samples %ld rejected %ld pixels %ld cells %ld lb_pos %ld ub_checked %ld tiles %ld raise_tiles %ld out %ld new_only %ld old_only %ld both_out %ld "
                "floor_in %ld control_cells %ld control_viol %ld\n",
                n_samples, n_rejected, n_pixels, n_cells, n_lb_pos, n_ub_checked, n_tiles, n_raise_tiles, n_out_at_wmax, n_new_only, n_old_only, n_both_out, n_floor_in,
                n_control_cells, n_control_viol);
    if (g_fail) { std::printf("%d violations\n", g_fail); return 1; }
    std::printf("cull slack ok\n");
    return 0;
}
