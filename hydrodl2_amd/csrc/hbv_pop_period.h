// hbv_pop_period.h -- population scores against period means (hbvx_population_period, include/hbvx.h): the launch of
// hbvx_population_joint with the routed flow and the aux flux averaged over the periods of two calendars -- 8-day
// composites, months -- before they meet their targets: the eight [P,B] sums run once per period instead of once per
// day, and the optional series are [P,K,B] period means.  The per-period arithmetic is hbvx_popk::PeriodMean,
// BasinStats::score and AuxStats::push (hbv_pop.h), which compile for the host (tests/hosttest/popperiod_host.cpp).
#pragma once

#include "hbv_pop.h"

#if defined(__HIPCC__)

namespace hbvx {

struct PopPeriodArgs {
    PopJointArgs j;             // the two terms: hbvx_population_joint's arguments, targets / weights / series per PERIOD
    int has_aux;                // 0: aux_series == HBVX_POP_NO_AUX, nothing of j's aux part is read or written
    int n_flow, n_aux;          // KF, KA
    const int *flow_end, *aux_end;      // [KF], [KA]: closing days relative to t_first, ascending
};

// ---------------------------------------------------------------------------
// k_pop_period<MODEL, BETAET, TR>: k_pop_joint with a PeriodMean between each value and its chains -- the same lanes,
// grid, candidate axis, day loop, prefetch of the forcings and dynamic rows and shared butterfly loop, the same y and v.
// A restatement once more (k_pop, k_pop_stats and k_pop_joint keep their text, registers and schedule); a change to the
// day loop belongs in all four.  tests/test_population_period_gpu.py holds this kernel under daily calendars to
// k_pop_joint's bits.
//
// Each calendar has a cursor k, the day its period opened and the day it closes, all relative to t_first and uniform
// over the wave (they come from kernel arguments and scalar loads).  A scored day adds to the period's accumulator; a
// day that closes a period divides once, runs the four chains against row k of the target, lets the leader store the
// mean, moves the cursor and loads the next closing day and the next period's target row and weight -- at the OPENING of
// the period that needs them, so that its close does not wait on memory; they have left the per-day prefetch.  A cursor
// stops at its count: no closing day and no target row beyond K is read, whatever the calendar holds.  A closing day
// that is not ahead of the cursor's day (a calendar that does not ascend) is never met: the periods from there on stay
// open, nothing else happens.  Days after the last closing day are simulated and scored nowhere.
//
// Without an aux term (has_aux == 0, uniform over the launch) the aux value is zero through the butterfly and nothing
// aux is accumulated, loaded or stored: the flow's operations are the same ones on the same values in both forms.
// ---------------------------------------------------------------------------
template <int MODEL, bool BETAET, int TR>
__global__ void __launch_bounds__(64) k_pop_period(const PopPeriodArgs Q)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const PopJointArgs &J = Q.j;
    const PopStatsArgs &S = J.s;
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
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20) ? d.elev[L.b] : 0.0f;

    float p[NPARAM_MAX];
    const float *dynp[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        const hbvx_pop_src &cs = pp.p[i];
        float v = cs.sta ? cs.sta[c * cs.c_stride + (int64_t)L.b * cs.b_stride + L.j]
                         : s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
        v = raw ? sigmoid_(v) : v;
        p[i] = descale_(v, s.lo, s.hi);
        dynp[i] = s.dyn ? s.dyn + (int64_t)L.b * s.dyn_b_stride + L.j : s.sta;
        use_dyn[i] = s.dyn && !(s.drop && s.drop[L.b]);
        if (s.dyn) dmask |= 1u << i;
    }
#pragma unroll
    for (int i = NP; i < NPARAM_MAX; i++) p[i] = 0.0f;

    float st[5];
#pragma unroll
    for (int k = 0; k < 5; k++) st[k] = d.state_in ? d.state_in[k * N + L.n] : 0.001f;

    hbvx_popk::BasinStats bs;
    bs.start(A.has_route != 0, S.shift[L.b], TR == hbvx_popk::T_LOG ? S.eps[L.b] : 0.0f);
    if (A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
    }

    const bool has_aux = Q.has_aux != 0;        // uniform over the launch
    hbvx_popk::AuxStats ax;
    ax.start(has_aux ? J.aux_shift[L.b] : 0.0f);
    const int aux_series = J.aux_series;

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const float act = L.active ? 1.0f : 0.0f;
    const int KF = Q.n_flow, KA = has_aux ? Q.n_aux : 0;
    const int *fend = Q.flow_end, *aend = Q.aux_end;
    const float *tg = pp.target + L.b;              // row k of [KF, B]: the TRANSFORMED target of period k
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim = pp.sim ? pp.sim + c * (int64_t)KF * d.B + L.b : nullptr;
    // the aux rows from the (scalar) bases with the lane's basin added per access, as in k_pop_joint
    const float *atg = J.aux_target;
    const float *awt = J.aux_w;
    float *asim = has_aux && J.aux_sim ? J.aux_sim + c * (int64_t)KA * d.B : nullptr;

    // the calendars' cursors (uniform): period kf of the flow runs from day sf to day ef of the scored days, ka / sa / ea
    // the same for the aux series; and the open periods' target rows and weights
    int kf = 0, sf = 0, ef = KF > 0 ? fend[0] : -1;
    int ka = 0, sa = 0, ea = KA > 0 ? aend[0] : -1;
    float obs = 0.0f, wobs = 1.0f, aobs = 0.0f, awobs = 1.0f;
    if (KF > 0) {
        obs = tg[0];
        if (wt) wobs = wt[0];
    }
    if (KA > 0) {
        aobs = atg[L.b];
        if (awt) awobs = awt[L.b];
    }
    hbvx_popk::PeriodMean pf, pa;
    pf.acc = pa.acc = 0.0f;

    // one-step-ahead register prefetch of the per-step inputs (k_fwd's)
    float nxf[3], nxd[NP];
    {
        const float *xr = xb;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][0] : 0.f;
    }

    for (int t = 0; t < T; t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
        }
#pragma unroll
        for (int i = 0; i < NP; i++)
            if ((dmask >> i) & 1) {
                float v = raw ? sigmoid_dyn_(cur[i]) : cur[i];
                float pv = descale_(v, d.p[i].lo, d.p[i].hi);
                if (use_dyn[i]) p[i] = pv;
            }
        s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
        s.template fwd<false, true>(p, nz, ac, elev, 0.f, 0.f);
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        // the ensemble mean of Q and the aux value, k_pop_joint's lines: two xor butterflies in one loop
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
        const float av = !has_aux ? 0.0f
                       : aux_series == HBVX_F_AET ? s.ET : aux_series == HBVX_F_SWE ? s.SP3
                       : aux_series == HBVX_F_Q0 ? s.Q0 : aux_series == HBVX_F_Q1 ? s.Q1 : s.Q2;
        float q = (mu ? s.Q * wq : s.Q) * act, v = av * act;
        for (int k = 0; k < lgMp; k++) {
            const float qo = __shfl_xor(q, 1 << k, 64), vo = __shfl_xor(v, 1 << k, 64);
            q += qo;
            v += vo;
        }
        if (!mu) q = q * invM;
        v = v * invM;
        const float y = bs.Basin::push(q, 0.0f, 0.0f, false);       // the routing runs every day
        const int rel = t - t_first;                                // the day among the scored days
        if (rel >= 0 && kf < KF) {
            pf.add(y, rel == sf);
            if (rel == ef) {
                const int n = ef - sf + 1;
                const float mean = n == 1 ? pf.acc : pf.close(n);       // (x / 1.0f is x: the same bits, no division)
                bs.template score<TR>(mean, obs, wobs);
                if (sim && L.leader) sim[(int64_t)kf * d.B] = mean;     // the mean, not its transform
                kf++;
                sf = rel + 1;
                if (kf < KF) {
                    ef = fend[kf];
                    obs = tg[(int64_t)kf * d.B];
                    if (wt) wobs = wt[(int64_t)kf * d.B];
                }
            }
        }
        if (rel >= 0 && ka < KA) {
            pa.add(v, rel == sa);
            if (rel == ea) {
                const int n = ea - sa + 1;
                const float mean = n == 1 ? pa.acc : pa.close(n);
                ax.push(mean, aobs, awobs);
                if (asim && L.leader) asim[(int64_t)ka * d.B + L.b] = mean;
                ka++;
                sa = rel + 1;
                if (ka < KA) {
                    ea = aend[ka];
                    aobs = atg[(int64_t)ka * d.B + L.b];
                    if (awt) awobs = awt[(int64_t)ka * d.B + L.b];
                }
            }
        }
    }
    if (L.leader) {
        const int64_t at = c * d.B + L.b;
        pp.cost[at] = bs.cost;
        S.s1[at] = bs.s1;
        S.s2[at] = bs.s2;
        S.s3[at] = bs.s3;
        if (has_aux) {
            J.aux_sse[at] = ax.sse;
            J.aux_s1[at] = ax.s1;
            J.aux_s2[at] = ax.s2;
            J.aux_s3[at] = ax.s3;
        }
    }
}

} // namespace hbvx

#endif // __HIPCC__
