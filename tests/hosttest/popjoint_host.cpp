// popjoint_host.cpp -- the per-basin part of hbvx_population_joint (hydrodl2_amd/csrc/hbv_pop.h: a BasinStats for the
// flow term and an AuxStats for the aux term) compiled for the host, one pair per basin fed day by day as k_pop's joint form
// feeds it (tests/test_popjoint_host.py).  Built together with popstats_host.cpp and pop_host.cpp, whose popstats_host
// (the BasinStats alone) the test holds the flow term to.
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

namespace {

template <int TR>
void run(int T, int B, int t_first, const float *a, const float *bb, const float *q, const float *target, const float *w,
         const float *shift, const float *eps, const float *v, const float *atarget, const float *aw, const float *ashift,
         float *y, float *out, float *aout)
{
    const int L = T < UH ? T : UH;
    for (int b = 0; b < B; b++) {
        BasinStats bs;
        bs.start(a != nullptr, shift[b], TR == T_LOG ? eps[b] : 0.0f);
        if (a) gamma_taps(a[b], bb[b], L, bs.uh);
        AuxStats ax;
        ax.start(ashift[b]);
        for (int t = 0; t < T; t++) {
            const bool counted = t >= t_first;
            const int64_t row = (int64_t)(t - t_first) * B + b;
            const float obs = counted ? target[row] : 0.0f;
            const float wt = (counted && w) ? w[row] : 1.0f;
            y[(int64_t)t * B + b] = bs.push<TR>(q[(int64_t)t * B + b], obs, wt, counted);
            if (counted) ax.push(v[(int64_t)t * B + b], atarget[row], aw ? aw[row] : 1.0f);
        }
        out[0 * B + b] = bs.cost;
        out[1 * B + b] = bs.s1;
        out[2 * B + b] = bs.s2;
        out[3 * B + b] = bs.s3;
        aout[0 * B + b] = ax.sse;
        aout[1 * B + b] = ax.s1;
        aout[2 * B + b] = ax.s2;
        aout[3 * B + b] = ax.s3;
    }
}

} // namespace

// The flow term's arguments are popstats_host's (q [T,B], a / bb [B] or nullptr, target ALREADY transformed and w
// [T - t_first, B], shift, eps [B]).  The aux term: v [T,B] the day's aux value (every day of the call; the days before
// t_first are not read), atarget and aw [T - t_first, B] (aw may be nullptr), ashift [B].  Out: y [T,B] the routed flow,
// out [4,B] = sse, s1, s2, s3 of the flow term, aout [4,B] the same of the aux term.  Returns 0, or -1 for an unknown
// transform.
extern "C" int popjoint_host(int T, int B, int t_first, int transform, const float *a, const float *bb, const float *q,
                             const float *target, const float *w, const float *shift, const float *eps, const float *v,
                             const float *atarget, const float *aw, const float *ashift, float *y, float *out, float *aout)
{
    switch (transform) {
    case T_NONE: run<T_NONE>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, y, out, aout); return 0;
    case T_SQRT: run<T_SQRT>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, y, out, aout); return 0;
    case T_LOG: run<T_LOG>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, y, out, aout); return 0;
    default: return -1;
    }
}
