// launch_stream_plan.h -- what the two streaming translation units share: admission of a problem to the streaming
// family (plan_stream), its grid-size cross-over, and the (model, BETAET, dynamic set) -> template dispatch.
// launch_stream.hip holds the forwards and the layout query, launch_stream_bwd.hip the adjoints: two units because each
// instantiates ~100 kernels (a header change cost 3.3 minutes of serial compile in one unit).
#pragma once
#include "hbvx_host.h"
#include "hbv_stream2.h"

namespace hbvx_host {
namespace stream_plan {
using namespace hbvx;

struct StreamPlan {
    bool ok;        // the streaming family can take this problem at all
    int lg;
    int64_t wgs;    // wavefronts of state
    int nd;
    int sc;         // dynamic set of hbv_stream2.h: 0 none, 1 / 2 compiled sets, 3 / 4 run-time list of <= 3 / <= 6 slots
    bool rows_ok;   // row trajectory: every offset fits 32 bits
    bool packed_ok; // packed trajectory / checkpoints: one day's rows fit 32 bits (descriptors rebased per day)
    int dslot[6];
};

inline StreamPlan plan_stream(const hbvx_desc *d)
{
    StreamPlan P{};
    P.lg = lg_members(d->M);
    const int bpw = 64 >> P.lg;
    P.wgs = ((int64_t)d->B + bpw - 1) / bpw;
    const int64_t N = (int64_t)d->B * d->M, lim = (int64_t)1 << 32;
    P.nd = count_dyn(d);
    const int nf = (d->model == HBVX_MODEL_HBV10) ? 11 : 12;
    P.ok = use_tiled(d) && env_int("HBVX_STREAM", 1) != 0 && P.nd <= STREAM2_LIST_MAX && !d->muwts && d->T > 0 &&
           (int64_t)nf * d->T * d->B * 4 < lim &&
           ((int64_t)d->T * d->x_t_stride + (int64_t)d->B * d->x_b_stride) * 4 < lim;
    unsigned mask = 0;
    int k = 0;
    for (int i = 0; i < d->n_param; i++)
        if (d->p[i].dyn) {
            mask |= 1u << i;
            if (k < 6) P.dslot[k++] = i;
            // one day's row per descriptor (the kernels rebase it every day): the tensor itself may exceed 4 GiB
            P.ok = P.ok && d->p[i].dyn_t_stride >= 0 && (int64_t)d->B * d->p[i].dyn_b_stride * 4 < lim;
        }
    const bool be = d->n_param >= 13;
    P.sc = mask == 0 ? 0
         : (mask == ((1u << P_BETA) | (1u << P_BETAET)) && be &&
            (d->model == HBVX_MODEL_HBV10 || d->model == HBVX_MODEL_HBV11P)) ? 1
         : (mask == ((1u << P_BETA) | (1u << P_K0) | (1u << P_BETAET)) &&
            (d->model == HBVX_MODEL_HBV20 || d->model == HBVX_MODEL_HOURLY)) ? 2 : (P.nd <= 3 ? 3 : 4);   // (nd <= 6: P.ok)
    if (env_int("HBVX_STREAM_SLOTLIST", 0) && P.sc > 0 && P.sc < 3) P.sc = 3;   // tests: the run-time list on a compiled set
    const int c0 = d->ch_prcp, c1 = d->ch_tmean, c2 = d->ch_pet;
    // a basin's three forcing values adjacent (one 12-byte load), the channels any permutation of {0, 1, 2} (the
    // kernels pick; config key `variables`).  Other layouts run the pipelined / tiled forward and their adjoints.
    P.ok = P.ok && (unsigned)c0 < 3u && (unsigned)c1 < 3u && (unsigned)c2 < 3u && c0 != c1 && c0 != c2 && c1 != c2 &&
           d->x_b_stride >= 3;
    P.rows_ok = 5 * (int64_t)(d->T + 1) * N * 4 < lim;
    P.packed_ok = N * 20 < lim;
    return P;
}

// Grid size (wavefronts of state) from which the streaming kernels run.  Measured on MI355X with
// tools/grid_sweep.py (profiles/r02_grid_sweep.jsonl): a training step (packed trajectory, both
// directions streaming) wins from 768 wavefronts for hbv and ties there for hbv_2; forward alone the
// pipelined kernel holds on to 1024.  HBVX_STREAM_MIN overrides both; HBVX_BWD=<family> pins the
// adjoint for tests.
inline int stream_min(bool training)
{
    return env_int("HBVX_STREAM_MIN", training ? 768 : 1024);
}
inline bool adjoint_pinned_elsewhere()
{
    const char *v = getenv("HBVX_BWD");
    return v && strcmp(v, "stream") != 0;
}

// (model, BETAET, dynamic set) -> f(model, BETAET, set), the three as std::integral_constant (with_model), for the
// instances hbv_stream2.h compiles: every model with none (0) and the run-time lists (3, 4); the compiled sets where
// plan_stream gives them, {BETA, BETAET} (1) to HBV 1.0 with BETAET and 1.1p, {BETA, K0, BETAET} (2) to 2.0 and hourly
template <typename F>
void with_stream2(const hbvx_desc *d, int sc, F &&f)
{
    with_model(d, [&](auto m, auto be) {
        constexpr bool S1 = be && (m == MODEL_HBV10 || m == MODEL_HBV11P), S2 = m == MODEL_HBV20 || m == MODEL_HOURLY;
        switch (sc) {
        case 0: f(m, be, std::integral_constant<int, 0>{}); break;
        case 1: if constexpr (S1) f(m, be, std::integral_constant<int, 1>{}); break;
        case 2: if constexpr (S2) f(m, be, std::integral_constant<int, 2>{}); break;
        case 3: f(m, be, std::integral_constant<int, 3>{}); break;
        default: f(m, be, std::integral_constant<int, 4>{}); break;
        }
    });
}

} // namespace stream_plan
} // namespace hbvx_host
