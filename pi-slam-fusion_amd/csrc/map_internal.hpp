// map_internal.hpp -- what the translation units of the map engine (fusion_map.cpp, map_*.cpp) share and nobody else sees
#pragma once
#include "map_support.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>

namespace pf {

#define HIP_OK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                  \
            return false;                                                                  \
        }                                                                                  \
    } while (0)

static inline int floordiv(int a, int b) { int q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) q--; return q; }

// a single-band tile's pixels (BGRA, Map2DCPU) as the three bytes the outputs carry
static inline void bgra_to_bgr(const uint8_t* bgra, uint8_t* bgr, size_t n)
{
    for (size_t i = 0; i < n; i++) { bgr[3 * i] = bgra[4 * i]; bgr[3 * i + 1] = bgra[4 * i + 1]; bgr[3 * i + 2] = bgra[4 * i + 2]; }
}

}  // namespace pf
