// popstats_host.cpp -- the per-basin part of hbvx_population_stats (hydrodl2_amd/csrc/hbv_pop.h: BasinStats -- Basin's
// window and routed value, the transform, the squared-error chain and the three moment chains about the shift)
// compiled for the host, one BasinStats per basin fed day by day as the kernel feeds it (tests/test_popstats_host.py).
// Built together with pop_host.cpp, whose pop_host (the Basin alone) the test holds this one to.
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

namespace {

template <int TR>
void run(int T, int B, int t_first, const float *a, const float *bb, const float *q, const float *target, const float *w,
         const float *shift, const float *eps, float *y, float *yt, float *out)
{
    const int L = T < UH ? T : UH;
    for (int b = 0; b < B; b++) {
        BasinStats bs;
        bs.start(a != nullptr, shift[b], TR == T_LOG ? eps[b] : 0.0f);
        if (a) gamma_taps(a[b], bb[b], L, bs.uh);
        for (int t = 0; t < T; t++) {
            const bool counted = t >= t_first;
            const int64_t row = (int64_t)(t - t_first) * B + b;
            const float obs = counted ? target[row] : 0.0f;
            const float wt = (counted && w) ? w[row] : 1.0f;
            const float v = bs.push<TR>(q[(int64_t)t * B + b], obs, wt, counted);
            y[(int64_t)t * B + b] = v;
            yt[(int64_t)t * B + b] = bs.transform<TR>(v);
        }
        out[0 * B + b] = bs.cost;
        out[1 * B + b] = bs.s1;
        out[2 * B + b] = bs.s2;
        out[3 * B + b] = bs.s3;
    }
}

} // namespace

// q [T,B] ensemble means; a, bb [B] physical route_a / route_b, or a == nullptr for the un-routed value; target (ALREADY
// transformed) and w [T - t_first, B], w may be nullptr; shift [B]; eps [B], read with transform 2 only.  Out: y [T,B]
// the routed value of every day, yt [T,B] its transform (what the chains saw on the counted days), out [4,B] = sse, s1,
// s2, s3.  Returns 0, or -1 for an unknown transform.
extern "C" int popstats_host(int T, int B, int t_first, int transform, const float *a, const float *bb, const float *q,
                             const float *target, const float *w, const float *shift, const float *eps, float *y,
                             float *yt, float *out)
{
    switch (transform) {
    case T_NONE: run<T_NONE>(T, B, t_first, a, bb, q, target, w, shift, eps, y, yt, out); return 0;
    case T_SQRT: run<T_SQRT>(T, B, t_first, a, bb, q, target, w, shift, eps, y, yt, out); return 0;
    case T_LOG: run<T_LOG>(T, B, t_first, a, bb, q, target, w, shift, eps, y, yt, out); return 0;
    default: return -1;
    }
}
