// undistort_plan_check.cpp -- csrc/undistort_plan.hpp alone, for a sanitizer build (tests/test_undistort_model.py): cameras given on the
// command line as "n p0 .. p(n-1) o0 .. o5", one line of output per camera pair:
//   <ok> <uncovered> <fnv1a of the x table's bits> <fnv1a of the y table's bits> <fit k>
// ok = 0 (and zeros) for a pair that is no camera.  The caller compares with what the library says.
#include "undistort_plan.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t fnv(const std::vector<float>& v)
{
    uint64_t h = 1469598103934665603ull;
    for (float f : v) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        for (int i = 0; i < 4; i++) { h ^= (b >> (8 * i)) & 0xff; h *= 1099511628211ull; }
    }
    return h;
}

int main(int argc, char** argv)
{
    int i = 1;
    while (i < argc) {
        const int n = std::atoi(argv[i++]);
        if (n < 0 || n > 16 || i + n + 6 > argc) return 2;
        std::vector<double> in, out;
        for (int k = 0; k < n; k++) in.push_back(std::strtod(argv[i++], nullptr));
        for (int k = 0; k < 6; k++) out.push_back(std::strtod(argv[i++], nullptr));
        pf::undistort::InCamera ic; pf::undistort::OutCamera oc;
        if (!pf::undistort::make_camera(in.data(), n, ic) || !pf::undistort::make_out_camera(out.data(), oc)) { std::printf("0 0 0 0 0\n"); continue; }
        std::vector<float> x((size_t)oc.w * oc.h), y(x.size());
        const long long unc = pf::undistort::build_table(ic, oc, x.data(), y.data());
        std::printf("1 %lld %llu %llu %d\n", unc, (unsigned long long)fnv(x), (unsigned long long)fnv(y), pf::undistort::fit_scale(ic, oc));
    }
    return 0;
}
