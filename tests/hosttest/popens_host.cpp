// popens_host.cpp -- the routing window of hbvx_population_ensemble across calls (hydrodl2_amd/csrc/hbv_pop.h:
// Basin::load_history / save_history) compiled for the host: one Basin per basin is given a history, pushed a run of days
// as the kernel pushes them, and asked for its history back (tests/test_popens_host.py).
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// q [n,B] the un-routed values of the run's days; a, bb [B] physical route_a / route_b; L the taps of the full record;
// hist_in [14,B] or nullptr (zeros).  Out: y [n,B] the routed values, hist_out [14,B].
extern "C" void popens_host(int n, int B, int L, const float *a, const float *bb, const float *q, const float *hist_in,
                            float *y, float *hist_out)
{
    for (int b = 0; b < B; b++) {
        Basin bs;
        bs.start(true);
        gamma_taps(a[b], bb[b], L, bs.uh);
        bs.load_history(hist_in ? hist_in + b : nullptr, B);
        for (int t = 0; t < n; t++) y[(int64_t)t * B + b] = bs.push(q[(int64_t)t * B + b], 0.0f, 0.0f, false);
        bs.save_history(hist_out + b, B);
    }
}
