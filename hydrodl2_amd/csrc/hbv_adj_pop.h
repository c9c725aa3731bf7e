// hbv_adj_pop.h -- population evaluation of the implicit scheme (hbvx_adj_population_cost / hbvx_adj_population_stats,
// include/hbvx.h): what hbv_pop.h does for the explicit models, with the day's Newton solve inside the day loop.  For
// every candidate static-parameter set and basin: the weighted squared error of the routed ensemble-mean streamflow
// (and, for the stats entry, the three moment chains of hbvx_popk::BasinStats), one launch, nothing else written.
//
// k_adj_pop<BETAET, FEW, TR> is k_adj_fwd's day loop (hbv_adj_kernels.h: the same day functions AdjStaged::day /
// adj_newton on the same parameter values, the same Q = (q0 + q1) + q2 at the solved state, the same ensemble sum)
// with k_pop's lane mapping and tail (hbv_pop.h: one wave per workgroup, blockIdx.x the wave's group of basins,
// blockIdx.y the CANDIDATE, one lane per (basin, member); gamma_taps, Basin / BasinStats, the leader stores).
//
// It RESTATES k_adj_fwd's lines and does not share a body with it: k_adj_fwd's registers and schedule are pinned
// (tools/compare_code.py), and every earlier attempt to pull shared text of these kernels into functions changed the
// callers' instructions (hbv_adj_kernels.h, the note above ADJ_STATIC_ROW).  What differs from k_adj_fwd:
//   - the static row comes from the candidate where pop.p[i].sta is set;
//   - the slot-list ("few") parameter fetch is used when the call has at most ADJ_FEW dynamic parameters: the generic
//     fetch costs a resident wave (see profiles/r17_adj_population.md);
//   - no trajectory, no state_out, no flux series: the mean goes into the basin's window and chains.
// A new kernel has no pinned history, so one body serves both entry points: TR = T_COST maps lanes onto
// hbvx_popk::Basin, T_NONE / T_SQRT / T_LOG onto BasinStats (k_pop and k_pop_stats are two texts for the reason given
// in hbv_pop.h).  Under T_NONE the cost chain is Basin's own operations on the same values: the same bits.
//
// adj_stop == 1 (the batch-wide stopping rule) is refused by the launcher: its voting set is the 64 lanes of the wave,
// so a candidate's cost would depend on which basins share its wave.  The kernel calls adj_newton with vote = false.
#pragma once

#include "hbv_adj_kernels.h"
#include "hbv_pop.h"

// 1: the forcings, the observation and its weight are loaded one day ahead of their use, as k_pop does
// (profiles/r17_adj_population.md has the measurement that settled it).
#ifndef ADJ_POP_PREFETCH
#define ADJ_POP_PREFETCH 1
#endif

namespace hbvx {

constexpr int T_COST = -1;      // TR of the cost-only instance (the others are hbvx_popk::T_*)

template <int TR> struct AdjPopBasin { using type = hbvx_popk::BasinStats; };
template <> struct AdjPopBasin<T_COST> { using type = hbvx_popk::Basin; };

template <bool BETAET, bool FEW, int TR>
__global__ void __launch_bounds__(64) k_adj_pop(const PopStatsArgs S, const AdjFew F)
{
    constexpr int NP = BETAET ? 13 : 12;
    constexpr bool STATS = TR != T_COST;
    const PopArgs &A = S.a;
    const hbvx_desc &d = A.d;
    const hbvx_pop &pp = A.pop;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int t_first = pp.t_first;
    const int64_t N = (int64_t)d.B * d.M;
    const int64_t c = blockIdx.y;
    const bool raw = d.raw_sigmoid != 0;
    const float invM = 1.0f / (float)d.M;

    // ADJ_STATIC_ROW's lines (hbv_adj_kernels.h) with the candidate's value where there is one; the drop masks are
    // per LANE and the recorded call's, shared by all candidates
    float usta[NP];                 // FEW: the static PHYSICAL values
    bool use_dyn[FEW ? ADJ_FEW : NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        const hbvx_pop_src &cs = pp.p[i];
        const float v = cs.sta ? cs.sta[c * cs.c_stride + (int64_t)L.b * cs.b_stride + L.j]
                               : s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
        usta[i] = raw ? sigmoid_(v) : v;
        if (FEW) usta[i] = descale_(usta[i], s.lo, s.hi);
        else use_dyn[i] = s.dyn && !(s.drop && s.drop[L.n]);
    }
    if (FEW) {
#pragma unroll
        for (int k = 0; k < ADJ_FEW; k++) {
            use_dyn[k] = false;
            if (k < F.nd) {
                const hbvx_param_src &s = d.p[F.slot[k]];
                use_dyn[k] = !(s.drop && s.drop[L.n]);
            }
        }
    }

    float x[5];
#pragma unroll
    for (int k = 0; k < 5; k++) x[k] = d.state_in ? d.state_in[k * N + L.n] : 0.0f;

    typename AdjPopBasin<TR>::type bs;
    if constexpr (STATS) bs.start(A.has_route != 0, S.shift[L.b], TR == hbvx_popk::T_LOG ? S.eps[L.b] : 0.0f);
    else bs.start(A.has_route != 0);
    if (A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs, as k_pop
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
    }

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *tg = pp.target + L.b;              // row t - t_first of [T - t_first, B]
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;

#if ADJ_POP_PREFETCH
    float nxf[3], nxo = 0.0f, nxw = 1.0f;
    if (T > 0) {
        nxf[0] = xb[d.ch_prcp]; nxf[1] = xb[d.ch_tmean]; nxf[2] = xb[d.ch_pet];
        if (t_first == 0) {
            nxo = tg[0];
            if (wt) nxw = wt[0];
        }
    }
#endif

    for (int t = 0; t < T; t++) {
        const bool counted = t >= t_first;
#if ADJ_POP_PREFETCH
        const float fP = nxf[0], fT = nxf[1], fE = nxf[2];
        const float obs = nxo, wobs = nxw;
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
            if (tn >= t_first) {
                const int64_t row = (int64_t)(tn - t_first) * d.B;
                nxo = tg[row];
                if (wt) nxw = wt[row];
            }
        }
#else
        const float *xr = xb + (int64_t)t * d.x_t_stride;
        const float fP = xr[d.ch_prcp], fT = xr[d.ch_tmean], fE = xr[d.ch_pet];
        float obs = 0.0f, wobs = 1.0f;
        if (counted) {
            const int64_t row = (int64_t)(t - t_first) * d.B;
            obs = tg[row];
            if (wt) wobs = wt[row];
        }
#endif
        float u[NP], p[NPARAM_MAX], xn[5];
        if (FEW) adj_params_few<NP>(d, L, t, raw, F, usta, use_dyn, u, p);
        else adj_params<NP>(d, L, t, raw, usta, use_dyn, u, p);
        AdjStep<BETAET> s;
        s.P = fP; s.Tf = fT; s.PET = fE;
        float Qs = 0.0f;
        if (d.adj_stop == 2) AdjStaged<BETAET>::day(p, s.P, s.Tf, s.PET, x, d.adj_gtol, d.adj_max_iter, xn, Qs);
        else adj_newton<BETAET>(s, p, x, 1.0f, d.adj_gtol, d.adj_max_iter, xn, false);
#pragma unroll
        for (int k = 0; k < 5; k++) x[k] = xn[k];
        // k_adj_fwd's lines: Q = q0 + q1 + q2 at the solved state, mean over members
        const float SUZ = fmaxf(x[3], 0.0f), SLZ = fmaxf(x[4], 0.0f);
        const float q0 = p[P_K0] * fmaxf(SUZ - p[P_UZL], 0.0f);
        const float q1 = p[P_K1] * SUZ, q2 = p[P_K2] * SLZ;
        float Q = (q0 + q1) + q2;
        Q = ens_sum(L.active ? Q : 0.0f, lgMp) * invM;
        float y;
        if constexpr (STATS) y = bs.template push<TR>(Q, obs, wobs, counted);
        else y = bs.push(Q, obs, wobs, counted);
        if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;      // y, not its transform
    }
    if (L.leader) {
        const int64_t at = c * d.B + L.b;
        pp.cost[at] = bs.cost;
        if constexpr (STATS) {
            S.s1[at] = bs.s1;
            S.s2[at] = bs.s2;
            S.s3[at] = bs.s3;
        }
    }
}

} // namespace hbvx
