// hbv_onepass_compose.h -- row layout and composition of the one-pass static adjoint's chunk maps (hbv_chunked.h,
// k_bwd_chunk_onepass).  Plain C++ on hbv_step.h's parameter slots, so that the same text compiles for gfx950 and for
// the host (tests/hosttest/onepass_compose_host.cpp runs it in double).
//
// A chunk c of a lane is the affine map
//     a_out[i] = phi[i] + sum_k a[k] Phi[k][i]        (adjoint entering the chunk from the future -> adjoint leaving it)
//     g[p]     = g0[p]  + sum_k G[k][p] a[k]          (the chunk's static-parameter gradient)
// Phi[k] is the propagated unit adjoint k.  Units 0 and 1 (SNOWPACK, MELTWATER) never leave the snow block, unit 2
// (SM) reaches snow and soil, units 3 and 4 everything: Phi[k][i] != 0 only for i < onepass_reach(k), and G[k][p] != 0
// only for k >= onepass_kmin(p).  Both patterns are closed under the composition below, so a composite has the rows of
// a single chunk.
#pragma once

#include "hbv_step.h"

#if defined(__HIPCC__)
#define HBVX_HDC __host__ __device__ constexpr
#else
#define HBVX_HDC constexpr
#endif
// Keeps the instruction scheduler from moving anything across this point (device code only).
#if defined(__HIP_DEVICE_COMPILE__)
#define HBVX_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define HBVX_SCHED_FENCE() ((void)0)
#endif

namespace hbvx {

HBVX_HDC int onepass_kmin(int i)
{
    return (i == P_TT || i == P_CFMAX || i == P_CFR || i == P_CWH) ? 0
         : ((i == P_BETA || i == P_FC || i == P_LP || i == P_BETAET) ? 2 : 3);
}
HBVX_HDC int onepass_row(int i)
{
    int r = 0;
    for (int j = 0; j < i; j++) r += 6 - onepass_kmin(j);
    return r;
}
HBVX_HDC int onepass_rows(int NP) { return onepass_row(NP); }
HBVX_HDC int onepass_reach(int k) { return k < 2 ? 2 : (k == 2 ? 3 : 5); }

// The rows of a map go to a sink (out.Phi(k, i, v), out.phi(i, v), out.G(k, p, v) with k == 5 for g0) and come from
// a source (L.Phi(k, j), L.phi(j), L.G(k, p)): registers -> LDS slot, LDS slot -> workspace rows, arrays on the host.
template <typename T, int NP, typename Dst>
HBVX_HDM void onepass_put(const T Phi[5][5], const T phi[5], const T G[6][NPARAM_MAX], Dst &out)
{
#pragma unroll
    for (int k = 0; k < 5; k++) {
        out.phi(k, phi[k]);
#pragma unroll
        for (int i = 0; i < 5; i++) out.Phi(k, i, Phi[k][i]);
    }
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int k = onepass_kmin(p); k < 6; k++) out.G(k, p, G[k][p]);
}

// Fold a later map L (chunk c+1, or the composite of everything later) into the earlier chunk E = (Phi, phi, G): the
// result maps the adjoint entering L to the adjoint leaving E and to the gradient of both.
//     Phi[k][i] = sum_j Phi_L[k][j] Phi_E[j][i]          phi[i] = phi_E[i] + sum_j phi_L[j] Phi_E[j][i]
//     G[k][p]   = G_L[k][p] + sum_j Phi_L[k][j] G_E[j][p]
//     g0[p]     = g0_L[p] + g0_E[p] + sum_j phi_L[j] G_E[j][p]           (g0 is row 5 of G)
// Only entries inside the sparsity patterns are read; those are written, and with DENSE the zeros of Phi too.
// The G / g0 lines sum in double whatever T is, one fused multiply-add per term: parPERC's SUZ and SLZ shares cancel in
// sum_j as they do in k_bwd_chunk_fold.  The Phi / phi lines are the scan's hop and stay in T.
// Every result leaves through the sink as soon as it is formed, Phi and phi first, then G column by column, and the
// sink may be the storage L is read from: an entry of L is read before the sink gets the entry of the same place.
// On the GPU this order is what keeps the registers down: E's values die as their columns are done, L's column of the
// next parameter is fetched while this one's is worked on, and a scheduling fence closes every column -- left alone,
// the compiler reads all of L at the top, where it meets all of E and the double copies of Phi_L (170 VGPRs instead
// of 156: the kernel's third wave per SIMD).
template <typename T, int NP, bool DENSE, typename Src, typename Dst>
HBVX_HDM void onepass_compose(const Src &L, const T Phi[5][5], const T phi[5], const T G[6][NPARAM_MAX], Dst &out)
{
    T PL[5][5], pl[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        pl[k] = L.phi(k);
#pragma unroll
        for (int j = 0; j < 5; j++) PL[k][j] = j < onepass_reach(k) ? L.Phi(k, j) : T(0);
    }
    HBVX_SCHED_FENCE();
#pragma unroll
    for (int i = 0; i < 5; i++) {
        T v = phi[i];
#pragma unroll
        for (int j = 0; j < 5; j++)
            if (i < onepass_reach(j)) v += pl[j] * Phi[j][i];
        out.phi(i, v);
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (i >= onepass_reach(k)) {
                if (DENSE) out.Phi(k, i, T(0));
                continue;
            }
            T s = T(0);
            bool first = true;
#pragma unroll
            for (int j = 0; j < 5; j++)
                if (j < onepass_reach(k) && i < onepass_reach(j)) {
                    s = first ? PL[k][j] * Phi[j][i] : s + PL[k][j] * Phi[j][i];
                    first = false;
                }
            out.Phi(k, i, s);
        }
    }
    T ln[6];
#pragma unroll
    for (int k = 0; k < 6; k++) ln[k] = k >= onepass_kmin(0) ? L.G(k, 0) : T(0);
    HBVX_SCHED_FENCE();
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int k0 = onepass_kmin(p);
        T lc[6];
#pragma unroll
        for (int k = 0; k < 6; k++) lc[k] = ln[k];
        if (p + 1 < NP) {
#pragma unroll
            for (int k = 0; k < 6; k++) ln[k] = k >= onepass_kmin(p + 1) ? L.G(k, p + 1) : T(0);
        }
        double ge[5];
#pragma unroll
        for (int j = 0; j < 5; j++) ge[j] = j >= k0 ? (double)G[j][p] : 0.0;
        double v0 = (double)lc[5] + (double)G[5][p];
#pragma unroll
        for (int j = 0; j < 5; j++)
            if (j >= k0) v0 = fma((double)pl[j], ge[j], v0);
        out.G(5, p, (T)v0);
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (k < k0) continue;
            double v = (double)lc[k];
#pragma unroll
            for (int j = 0; j < 5; j++)
                if (j >= k0 && j < onepass_reach(k)) v = fma((double)PL[k][j], ge[j], v);
            out.G(k, p, (T)v);
        }
        HBVX_SCHED_FENCE();
    }
}

} // namespace hbvx
