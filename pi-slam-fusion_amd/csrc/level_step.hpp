// level_step.hpp -- ONE step of the dependence recurrence of the collapse: pyrUp is a 3-tap filter, so pixels [lo, hi] of level i-1
// need pixels [(lo-1)>>1, (hi>>1)+1] of level i, clamped to the level's n pixels.  Plain integer code without a HIP header: the
// collapse kernels walk it for the regions a block holds in LDS (collapse_common.hpp, level_region), the view plan walks it on the
// host for the tiles a view depends on (view_plan.hpp).
#pragma once
#include "warp_index.hpp"          // PF_HD

namespace pf {

PF_HD void level_step(int& lo, int& hi, int n)
{
    lo = (lo - 1) >> 1; if (lo < 0) lo = 0;
    hi = (hi >> 1) + 1; if (hi > n - 1) hi = n - 1;
}

}  // namespace pf
