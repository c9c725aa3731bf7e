// hbv_gram.h -- per-basin normal equations of C series on a [T,B] grid (hbvx_gram, include/hbvx.h):
//   gram[b,c,e] = sum_t w s_c s_e,  rhs[b,c] = sum_t w s_c r,  cost[b] = sum_t w r^2.
// Everything a lane does -- the indexing, the time slicing, the order of every sum -- is in this header and compiles
// for the host as well (tests/hosttest/gram_host.cpp), so the CPU tier checks it without a GPU; the kernels in
// gram.hip only map lanes onto these functions.
//
// Form: lane = basin.  The series are direction-major [C,T,B], the basin is the unit-stride axis, so a wave's load of
// one (column, day) is one coalesced 256-byte row.  A wave holds TILE x TILE blocks of column pairs (I, J), I <= J, in
// registers and feeds them with plain fused multiply-adds; the waves of a workgroup share the columns of a block pair
// through LDS (gram.hip), which changes where an operand comes from and nothing about the sums.
//
// Order of the sums (what makes the result reproducible):
//   * the days are cut into S slices of L days, S and L functions of (T, B) alone (time_slices) -- never of C or of
//     the column tiling;
//   * inside a slice an element (c, e), c <= e, is ONE chain  acc = fmaf(w * s_c, s_e, acc)  over ascending t from 0
//     (w * s_c rounded once; without w it is s_c itself);
//   * pass two adds the S slice sums in ascending order, starting from slice 0's;
//   * only c <= e is ever computed; gram[b,e,c] is a copy of gram[b,c,e].
// So the bits of gram[b,c,e] depend on the two series, the weights and (T, B) -- not on which other columns exist
// (removing columns keeps the order of the remaining ones, hence which of the pair is weighted).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HBVX_GRAM_HD __host__ __device__ __forceinline__
#else
#define HBVX_GRAM_HD inline
#endif

namespace hbvx_gramk {

constexpr int TILE = 8;              // columns per register tile side
constexpr int TT = TILE * TILE;
constexpr int BLOCK = 4;             // tiles per side of a workgroup's column block: 32 x 32 columns from 64 staged ones
#ifndef HBVX_GRAM_UNITS
#define HBVX_GRAM_UNITS 128          // A/B builds only (python __graft_entry__.py variant <tag> -DHBVX_GRAM_UNITS=...)
#endif
constexpr int UNITS = HBVX_GRAM_UNITS;   // (basin group, slice) units wanted: with 671 basins there are only 11 groups
constexpr int MIN_SLICE = 32;        // days: a shorter slice is not worth a workspace row

struct Plan {
    int T, B, C;
    int G;            // basin groups of 64
    int S, L;         // slices, days per slice (the last one may be shorter)
    int NT;           // column tiles
    int64_t NPAIR;    // tile pairs I <= J
    int NB;           // column blocks of BLOCK tiles
    int NWG;          // workgroups per unit: block pairs BI <= BJ
};

HBVX_GRAM_HD void time_slices(int T, int B, int *S, int *L)
{
    const int G = (B + 63) / 64;
    const int want = (UNITS + G - 1) / G;
    int len = (T + want - 1) / want;
    if (len < MIN_SLICE) len = MIN_SLICE;
    *L = len;
    *S = (T + len - 1) / len;
}

HBVX_GRAM_HD Plan make_plan(int T, int B, int C)
{
    Plan p;
    p.T = T; p.B = B; p.C = C;
    p.G = (B + 63) / 64;
    time_slices(T, B, &p.S, &p.L);
    p.NT = (C + TILE - 1) / TILE;
    p.NPAIR = (int64_t)p.NT * (p.NT + 1) / 2;
    p.NB = (p.NT + BLOCK - 1) / BLOCK;
    p.NWG = p.NB * (p.NB + 1) / 2;
    return p;
}

// index of tile pair (I, J), I <= J, among the NPAIR
HBVX_GRAM_HD int64_t pair_index(int NT, int I, int J) { return (int64_t)I * NT - (int64_t)I * (I - 1) / 2 + (J - I); }

// workgroup `wg` of a unit -> its block pair BI <= BJ (row-major over the upper triangle)
HBVX_GRAM_HD void workgroup_blocks(int NB, int wg, int *BI, int *BJ)
{
    int i = 0;
    for (; i < NB - 1 && wg >= NB - i; i++) wg -= NB - i;
    *BI = i;
    *BJ = i + wg;
}

// Workspace (floats): slice sums, the basin innermost so that lanes store coalesced.
//   gram part [S][NPAIR][TT][B], then rhs part [S][C][B], then cost part [S][B]
HBVX_GRAM_HD int64_t ws_gram_floats(const Plan &p) { return (int64_t)p.S * p.NPAIR * TT * p.B; }
HBVX_GRAM_HD int64_t ws_rhs_floats(const Plan &p) { return (int64_t)p.S * p.C * p.B; }
HBVX_GRAM_HD int64_t ws_cost_floats(const Plan &p) { return (int64_t)p.S * p.B; }
HBVX_GRAM_HD int64_t ws_floats(const Plan &p) { return ws_gram_floats(p) + ws_rhs_floats(p) + ws_cost_floats(p); }
HBVX_GRAM_HD int64_t ws_gram_at(const Plan &p, int sl, int64_t pair, int ij, int b)
{
    return (((int64_t)sl * p.NPAIR + pair) * TT + ij) * p.B + b;
}
HBVX_GRAM_HD int64_t ws_rhs_at(const Plan &p, int sl, int c, int b) { return ((int64_t)sl * p.C + c) * p.B + b; }
HBVX_GRAM_HD int64_t ws_cost_at(const Plan &p, int sl, int b) { return (int64_t)sl * p.B + b; }

// The arithmetic of one lane and one tile pair over a chunk of up to DAYS consecutive days (what the kernel holds in
// registers at a time).  a[i][k] = w * s_c(i) of day k (rounded once; s itself without weights), v[k] = s_e(j) of day k.
// Every element keeps ONE chain over ascending days, whatever the chunking.
constexpr int DAYS = 4;

template <bool DIAG>
HBVX_GRAM_HD void column_days(int nd, const float (&a)[TILE][DAYS], const float (&v)[DAYS], int j, float (&acc)[TILE][TILE])
{
    if (nd == DAYS) {                   // a whole chunk: no test per day (the same operations in the same order)
#pragma unroll
        for (int k = 0; k < DAYS; k++)
#pragma unroll
            for (int i = 0; i < TILE; i++)
                if (!DIAG || i <= j) acc[i][j] = __builtin_fmaf(a[i][k], v[k], acc[i][j]);
        return;
    }
#pragma unroll
    for (int k = 0; k < DAYS; k++)
        if (k < nd) {
#pragma unroll
            for (int i = 0; i < TILE; i++)
                if (!DIAG || i <= j) acc[i][j] = __builtin_fmaf(a[i][k], v[k], acc[i][j]);
        }
}

HBVX_GRAM_HD void rhs_days(int nd, const float (&a)[TILE][DAYS], const float (&rv)[DAYS], float (&rh)[TILE])
{
#pragma unroll
    for (int k = 0; k < DAYS; k++)
        if (k < nd) {
#pragma unroll
            for (int i = 0; i < TILE; i++) rh[i] = __builtin_fmaf(a[i][k], rv[k], rh[i]);
        }
}

template <bool HAS_W>
HBVX_GRAM_HD void cost_days(int nd, const float (&wv)[DAYS], const float (&rv)[DAYS], float &cost)
{
#pragma unroll
    for (int k = 0; k < DAYS; k++)
        if (k < nd) cost = __builtin_fmaf(HAS_W ? wv[k] * rv[k] : rv[k], rv[k], cost);
}

// The slice sums of one lane and one tile pair go to the workspace.  Columns past C have been summed on clamped loads;
// they are stored (the workspace has the room) and never read.  In a diagonal tile only i <= j is stored.
template <bool DIAG>
HBVX_GRAM_HD void store_tile(const Plan &p, float *ws, int sl, int b, int I, int J, const float (&acc)[TILE][TILE])
{
    const int64_t pair = pair_index(p.NT, I, J);
#pragma unroll
    for (int i = 0; i < TILE; i++)
#pragma unroll
        for (int j = 0; j < TILE; j++)
            if (!DIAG || i <= j) ws[ws_gram_at(p, sl, pair, i * TILE + j, b)] = acc[i][j];
}

HBVX_GRAM_HD void store_rhs(const Plan &p, float *ws, int sl, int b, int I, const float (&rh)[TILE], float cost)
{
    float *wr = ws + ws_gram_floats(p);
#pragma unroll
    for (int i = 0; i < TILE; i++)
        if (I * TILE + i < p.C) wr[ws_rhs_at(p, sl, I * TILE + i, b)] = rh[i];
    if (I == 0) wr[ws_rhs_floats(p) + ws_cost_at(p, sl, b)] = cost;
}

// Pass one for one lane and one tile pair straight from memory: slice `sl`, basin `b` (< B: the caller clamps a tail
// lane and passes store = false).  The kernel does the same arithmetic on operands it has staged in LDS; this is the
// form the host test runs, and the statement of what the kernel computes.
template <bool DIAG, bool HAS_W, bool HAS_R>
HBVX_GRAM_HD void lane_partial(const Plan &p, const float *s, int64_t series_stride, const float *w, const float *r,
                               float *ws, int sl, int b, bool store, int I, int J)
{
    const float *si[TILE], *sj[TILE];
#pragma unroll
    for (int i = 0; i < TILE; i++) {
        int c = I * TILE + i, e = J * TILE + i;
        c = c < p.C ? c : p.C - 1;
        e = e < p.C ? e : p.C - 1;
        si[i] = s + (int64_t)c * series_stride + b;
        sj[i] = s + (int64_t)e * series_stride + b;
    }
    float acc[TILE][TILE], rh[TILE], cost = 0.0f;
#pragma unroll
    for (int i = 0; i < TILE; i++) {
        rh[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < TILE; j++) acc[i][j] = 0.0f;
    }
    const int t0 = sl * p.L;
    const int t1 = t0 + p.L < p.T ? t0 + p.L : p.T;
    for (int t = t0; t < t1; t += DAYS) {
        const int nd = t1 - t < DAYS ? t1 - t : DAYS;
        float a[TILE][DAYS], wv[DAYS], rv[DAYS];
        for (int k = 0; k < DAYS; k++) {
            const int64_t off = (int64_t)(t + k < t1 ? t + k : t1 - 1) * p.B;
            wv[k] = HAS_W ? w[off + b] : 1.0f;
            rv[k] = HAS_R ? r[off + b] : 0.0f;
            for (int i = 0; i < TILE; i++) a[i][k] = HAS_W ? wv[k] * si[i][off] : si[i][off];
        }
        for (int j = 0; j < TILE; j++) {
            float v[DAYS];
            for (int k = 0; k < DAYS; k++) v[k] = sj[j][(int64_t)(t + k < t1 ? t + k : t1 - 1) * p.B];
            column_days<DIAG>(nd, a, v, j, acc);
        }
        if (HAS_R && DIAG) {
            rhs_days(nd, a, rv, rh);
            if (I == 0) cost_days<HAS_W>(nd, wv, rv, cost);
        }
    }
    if (!store) return;
    store_tile<DIAG>(p, ws, sl, b, I, J, acc);
    if (HAS_R && DIAG) store_rhs(p, ws, sl, b, I, rh, cost);
}

// Pass two: the S slice sums of one element in ascending order.  `part` points at slice 0's value, slices are
// `slice_stride` floats apart.
HBVX_GRAM_HD float ordered_sum(const float *part, int S, int64_t slice_stride)
{
    float v = part[0];
    for (int sl = 1; sl < S; sl++) v += part[(int64_t)sl * slice_stride];
    return v;
}

// element ij = i * TILE + j of tile pair (I, J) as the workspace holds it: a diagonal tile keeps i <= j only
HBVX_GRAM_HD int stored_ij(bool diag, int i, int j) { return (diag && i > j) ? j * TILE + i : i * TILE + j; }

} // namespace hbvx_gramk
