// hbv_adj_pop.h -- population evaluation of the implicit scheme (hbvx_adj_population_cost / hbvx_adj_population_stats /
// hbvx_adj_population_period, include/hbvx.h): what hbv_pop.h does for the explicit models, with the day's Newton solve
// inside the day loop.  For every candidate static-parameter set and basin: the weighted squared error of the routed
// ensemble-mean streamflow (and, for the stats entry, the three moment chains of hbvx_popk::BasinStats; for the period
// entry, those against period means, with an optional observed STORAGE beside streamflow), one launch, nothing else
// written.
//
// k_adj_pop<BETAET, FEW, TR, AUX, Args> is k_adj_fwd's day loop (hbv_adj_kernels.h: the same day functions
// AdjStaged::day / adj_newton on the same parameter values, the same Q = (q0 + q1) + q2 at the solved state, the same
// ensemble sum) with k_pop's lane mapping and tail (hbv_pop.h: one wave per workgroup, blockIdx.x the wave's group of
// basins, blockIdx.y the CANDIDATE, one lane per (basin, member); gamma_taps, Basin / BasinStats, the leader stores).
//
// It RESTATES k_adj_fwd's lines and does not share a body with it: k_adj_fwd's registers and schedule are pinned
// (tools/compare_code.py), and every earlier attempt to pull shared text of these kernels into functions changed the
// callers' instructions (hbv_adj_kernels.h, the note above ADJ_STATIC_ROW).  What differs from k_adj_fwd:
//   - the static row comes from the candidate where pop.p[i].sta is set;
//   - the slot-list ("few") parameter fetch is used when the call has at most ADJ_FEW dynamic parameters: the generic
//     fetch costs a resident wave (see profiles/r17_adj_population.md);
//   - no trajectory, no state_out, no flux series: the mean goes into the basin's window and chains;
//   - the forcings, and in the daily form the observation and its weight, are loaded one day ahead of their use, as
//     k_pop does (profiles/r17_adj_population.md has the measurement that settled it).
//
// Args = PopStatsArgs serves the cost and the stats entry points: TR = T_COST maps lanes onto hbvx_popk::Basin, T_NONE /
// T_SQRT / T_LOG onto BasinStats.  Under T_NONE the cost chain is Basin's own operations on the same values: the same
// bits.  AUX is false.
//
// Args = PopPeriodArgs (PERIOD) carries k_pop's calendars around the same day loop: per calendar a cursor, the day its
// period opened and the day it closes, uniform over the wave; a scored day adds to a hbvx_popk::PeriodMean (the first
// day of a period assigns), the closing day divides once (a one-day period takes the day's value, no division), runs
// BasinStats::score<TR> (flow) or AuxStats::push (aux) against row k of the target and lets the leader store the mean;
// the next closing day, target row and weight are loaded when a period OPENS, they are not in the per-day prefetch.  A
// cursor stops at its count; a calendar that does not ascend only leaves periods unclosed; days after the last closing
// day are simulated and scored nowhere.  The routing runs every day.  The implicit scheme carries its five storages as
// the unknowns of every day's solve, so an observed snow pack or soil moisture is in the lane's registers each day: the
// aux value of day t is the ensemble mean of x[k] after the solve, k = 0..4 for SNOWPACK, MELTWATER, SM, SUZ, SLZ -- the
// RAW x[k], as k_adj_fwd writes it to its trajectory, not the fmaxf-clamped value that enters Q; its mean takes 1 / M,
// is never routed and never transformed, and goes through the same butterfly loop as Q (as k_pop's does).  AUX = false
// is an instance of its own: the registers of the aux chains (a PeriodMean, the four sums, the shift, a target and a
// weight) would cost the daily form's third resident wave (profiles/r20_adj_population_period.md has every instance's
// count).  The flow's operations are the same ones on the same values in every form
// (tests/test_adj_population_period_gpu.py holds the period form under daily calendars to the daily form's bits).
//
// As for k_pop, every instance is instruction for instruction the kernel it had when the two forms were two texts
// (profiles/r21_population_one_source.md), and the forms keep the statement shapes that takes: the daily form leaves the
// prefetched forcings `nxf` uninitialised, the period form clears them with ONE block fill (what its `= {0, 0, 0}`
// compiled to; three element stores order the loop's phis the other way round and move 16 to 88 instructions per period
// instance); and the aux arguments are read through a
// `const PopJointArgs &`, not as `Q.j.x` (the access path is part of the load's alias tag).
//
// adj_stop == 1 (the batch-wide stopping rule) is refused by the launcher: its voting set is the 64 lanes of the wave,
// so a candidate's cost would depend on which basins share its wave.  The kernel calls adj_newton with vote = false.
#pragma once

#include "hbv_adj_kernels.h"
#include "hbv_pop.h"

namespace hbvx {

template <bool BETAET, bool FEW, int TR, bool AUX, typename Args>
__global__ void __launch_bounds__(64) k_adj_pop(const Args Q, const AdjFew F)
{
    constexpr int NP = BETAET ? 13 : 12;
    constexpr bool STATS = TR != T_COST;
    constexpr bool PERIOD = std::is_same<Args, PopPeriodArgs>::value;
    static_assert(PERIOD ? STATS : !AUX, "the period form has no cost-only instance, the daily form no aux term");
    const PopStatsArgs &S = stats_args(Q);
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

    typename PopBasin<TR>::type bs;
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

    hbvx_popk::AuxStats ax;
    int aux_k = 0;              // 0..4 with AUX: which storage (the launcher checked it)
    if constexpr (PERIOD) {
        const PopJointArgs &J = joint_args(Q);
        ax.start(AUX ? J.aux_shift[L.b] : 0.0f);
        aux_k = J.aux_series;
    }

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    int KF = 0, KA = 0;                             // PERIOD: the calendars' lengths and closing days
    const int *fend = nullptr, *aend = nullptr;
    if constexpr (PERIOD) {
        KF = Q.n_flow, KA = AUX ? Q.n_aux : 0;
        fend = Q.flow_end, aend = Q.aux_end;
    }
    // row t - t_first of [T - t_first, B], PERIOD: row k of [KF, B]; with STATS the TRANSFORMED target
    const float *tg = pp.target + L.b;
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim;
    if constexpr (PERIOD) sim = pp.sim ? pp.sim + c * (int64_t)KF * d.B + L.b : nullptr;
    else sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;
    // the aux rows from the (scalar) bases with the lane's basin added per access, as in k_pop
    const float *atg = nullptr, *awt = nullptr;
    float *asim = nullptr;
    if constexpr (PERIOD) {
        const PopJointArgs &J = joint_args(Q);
        atg = J.aux_target;
        awt = J.aux_w;
        asim = AUX && J.aux_sim ? J.aux_sim + c * (int64_t)KA * d.B : nullptr;
    }

    // PERIOD: the calendars' cursors (uniform) and the open periods' target rows and weights, k_pop's lines
    int kf = 0, sf = 0, ef = KF > 0 ? fend[0] : -1;
    int ka = 0, sa = 0, ea = KA > 0 ? aend[0] : -1;
    float pobs = 0.0f, pwobs = 1.0f, paobs = 0.0f, pawobs = 1.0f;
    hbvx_popk::PeriodMean pf, pa;
    if constexpr (PERIOD) {
        if (KF > 0) {
            pobs = tg[0];
            if (wt) pwobs = wt[0];
        }
        if (AUX && KA > 0) {
            paobs = atg[L.b];
            if (awt) pawobs = awt[L.b];
        }
        pf.acc = pa.acc = 0.0f;
    }

    // the forcings one day ahead of their use, and in the daily form the observation and its weight with them (the
    // period form's are per period: loaded at the openings)
    float nxf[3], nxo = 0.0f, nxw = 1.0f;
    if constexpr (PERIOD) __builtin_memset(nxf, 0, sizeof nxf);
    if (T > 0) {
        nxf[0] = xb[d.ch_prcp]; nxf[1] = xb[d.ch_tmean]; nxf[2] = xb[d.ch_pet];
        if constexpr (!PERIOD) {
            if (t_first == 0) {
                nxo = tg[0];
                if (wt) nxw = wt[0];
            }
        }
    }

    for (int t = 0; t < T; t++) {
        const bool counted = t >= t_first;
        const float fP = nxf[0], fT = nxf[1], fE = nxf[2];
        const float obs = nxo, wobs = nxw;
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
            if constexpr (!PERIOD) {
                if (tn >= t_first) {
                    const int64_t row = (int64_t)(tn - t_first) * d.B;
                    nxo = tg[row];
                    if (wt) nxw = wt[row];
                }
            }
        }
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
        float q = (q0 + q1) + q2;
        float v = 0.0f;
        if constexpr (AUX) {
            // the raw solved storage, as k_adj_fwd's trajectory holds it; both means in one butterfly loop (ens_sum's
            // operations on each value, as k_pop)
            const float av = aux_k == 0 ? x[0] : aux_k == 1 ? x[1] : aux_k == 2 ? x[2] : aux_k == 3 ? x[3] : x[4];
            q = L.active ? q : 0.0f;
            v = L.active ? av : 0.0f;
            for (int k = 0; k < lgMp; k++) {
                const float qo = __shfl_xor(q, 1 << k, 64), vo = __shfl_xor(v, 1 << k, 64);
                q += qo;
                v += vo;
            }
            q = q * invM;
            v = v * invM;
        } else {
            q = ens_sum(L.active ? q : 0.0f, lgMp) * invM;
        }
        if constexpr (PERIOD) {
            const float y = bs.Basin::push(q, 0.0f, 0.0f, false);       // the routing runs every day
            const int rel = t - t_first;                                // the day among the scored days
            if (rel >= 0 && kf < KF) {
                pf.add(y, rel == sf);
                if (rel == ef) {
                    const int n = ef - sf + 1;
                    const float mean = n == 1 ? pf.acc : pf.close(n);       // (x / 1.0f is x: the same bits, no division)
                    bs.template score<TR>(mean, pobs, pwobs);
                    if (sim && L.leader) sim[(int64_t)kf * d.B] = mean;     // the mean, not its transform
                    kf++;
                    sf = rel + 1;
                    if (kf < KF) {
                        ef = fend[kf];
                        pobs = tg[(int64_t)kf * d.B];
                        if (wt) pwobs = wt[(int64_t)kf * d.B];
                    }
                }
            }
            if constexpr (AUX) {
                if (rel >= 0 && ka < KA) {
                    pa.add(v, rel == sa);
                    if (rel == ea) {
                        const int n = ea - sa + 1;
                        const float mean = n == 1 ? pa.acc : pa.close(n);
                        ax.push(mean, paobs, pawobs);
                        if (asim && L.leader) asim[(int64_t)ka * d.B + L.b] = mean;
                        ka++;
                        sa = rel + 1;
                        if (ka < KA) {
                            ea = aend[ka];
                            paobs = atg[(int64_t)ka * d.B + L.b];
                            if (awt) pawobs = awt[(int64_t)ka * d.B + L.b];
                        }
                    }
                }
            }
        } else {
            float y;
            if constexpr (STATS) y = bs.template push<TR>(q, obs, wobs, counted);
            else y = bs.push(q, obs, wobs, counted);
            if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;      // y, not its transform
        }
    }
    if (L.leader) {
        const int64_t at = c * d.B + L.b;
        pp.cost[at] = bs.cost;
        if constexpr (STATS) {
            S.s1[at] = bs.s1;
            S.s2[at] = bs.s2;
            S.s3[at] = bs.s3;
        }
        if constexpr (AUX) {
            const PopJointArgs &J = joint_args(Q);
            J.aux_sse[at] = ax.sse;
            J.aux_s1[at] = ax.s1;
            J.aux_s2[at] = ax.s2;
            J.aux_s3[at] = ax.s3;
        }
    }
}

} // namespace hbvx
