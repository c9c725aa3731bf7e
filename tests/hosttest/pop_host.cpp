// pop_host.cpp -- the per-basin part of hbvx_population_cost (hydrodl2_amd/csrc/hbv_pop.h: unit hydrograph, 15-day
// window, causal convolution, residual chain) compiled for the host, one Basin per basin fed day by day as the
// kernel feeds it (tests/test_pop_host.py).
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// q [T,B] ensemble means; a, bb [B] physical route_a / route_b, or a == nullptr for the un-routed cost; target and w
// [T - t_first, B], w may be nullptr.  Out: uh [B,15] the taps used, y [T,B] the value every day produced (days before
// t_first included), cost [B].
extern "C" void pop_host(int T, int B, int t_first, const float *a, const float *bb, const float *q, const float *target,
                         const float *w, float *uh, float *y, float *cost)
{
    const int L = T < UH ? T : UH;
    for (int b = 0; b < B; b++) {
        Basin bs;
        bs.start(a != nullptr);
        if (a) gamma_taps(a[b], bb[b], L, bs.uh);
        for (int k = 0; k < UH; k++) uh[b * UH + k] = bs.uh[k];
        for (int t = 0; t < T; t++) {
            const bool counted = t >= t_first;
            const int64_t row = (int64_t)(t - t_first) * B + b;
            const float obs = counted ? target[row] : 0.0f;
            const float wt = (counted && w) ? w[row] : 1.0f;
            y[(int64_t)t * B + b] = bs.push(q[(int64_t)t * B + b], obs, wt, counted);
        }
        cost[b] = bs.cost;
    }
}
