// hbv_quadform.h -- per-basin quadratic form of C series on a [T,B] grid (hbvx_quadform, include/hbvx.h):
//   q[t,b] = | M_b s[:,t,b] |^2 = s^T (M_b^T M_b) s,   M_b lower-triangular [C,C].
// Everything a lane does -- the indexing, the packed factor, the order of every sum -- is in this header and compiles
// for the host as well (tests/hosttest/quadform_host.cpp), so the CPU tier checks it without a GPU; the kernels in
// quadform.hip only map lanes onto these functions.
//
// Definition (float32, per (t, b)):
//   y_e = chain over ascending c = 0..e :    acc = fmaf(m[b,e,c], s[c,t,b], acc), from 0
//   q   = chain over ascending e = 0..C-1 :  q = fmaf(y_e, y_e, q), from 0
// Both chains belong to one (t, b) alone, so the bits of q[t,b] depend on m[b] and s[:,t,b] and on nothing else: not on
// T, B, the stride between the series, the other days or basins, or the tiling below.
//
// Form: lane = basin.  The series are direction-major [C,T,B], the basin is the unit-stride axis, so a wave's load of
// one (column, day) is one coalesced 256-byte row.  The factor is per basin, hence per lane: pass one repacks its lower
// triangle into the workspace with the basin innermost, [C(C+1)/2][B], after which a wave's load of one m[e,c] is a
// coalesced row too.  A wave then owns (basin group of 64, QDAYS consecutive days) and walks the rows e in tiles of
// QROWS: a QROWS x QDAYS register tile of y is fed over ascending c -- each packed factor row serves QDAYS days, each
// series row QROWS factor rows -- then squared and added to q in ascending e.  q never leaves the lane's registers, so
// the chain over e needs no exchange between waves and no atomics.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HBVX_QF_HD __host__ __device__ __forceinline__
#else
#define HBVX_QF_HD inline
#endif

namespace hbvx_qfk {

constexpr int QROWS = 8;             // factor rows e per register tile
constexpr int QDAYS = 8;             // days per wave

// rows 0..e-1 of the lower triangle hold e(e+1)/2 elements
HBVX_QF_HD int64_t tri(int e) { return (int64_t)e * (e + 1) / 2; }

// Workspace (floats): the lower triangle of every basin's factor, the basin innermost: [C(C+1)/2][B]
HBVX_QF_HD int64_t ws_floats(int B, int C) { return tri(C) * B; }
HBVX_QF_HD int64_t packed_at(int B, int e, int c, int b) { return (tri(e) + c) * B + b; }     // c <= e
HBVX_QF_HD int64_t factor_at(int C, int b, int e, int c) { return ((int64_t)b * C + e) * C + c; }

// Pass one, the turn through LDS of one workgroup (basin group g, factor row e, columns c0 .. c0 + PACK - 1): element i of
// PACK * PACK is READ along the factor row (c the unit-stride axis of m) into tile[c - c0][basin - 64 g] and WRITTEN along
// the basins (the unit-stride axis of the packed triangle).  Only c <= e is touched, by both halves alike.
constexpr int PACK = 64;             // basins of a group = columns per turn
constexpr int PACK_PITCH = PACK + 1; // floats per tile row: a wave's 64 writes of one basin fall on 64 banks

HBVX_QF_HD void pack_read(int B, int C, int g, int e, int c0, int i, const float *m, float (*tile)[PACK_PITCH])
{
    const int bl = i / PACK, cc = i % PACK;
    const int b = g * PACK + bl, c = c0 + cc;
    if (b < B && c <= e) tile[cc][bl] = m[factor_at(C, b, e, c)];
}

HBVX_QF_HD void pack_write(int B, int g, int e, int c0, int i, const float (*tile)[PACK_PITCH], float *packed)
{
    const int cc = i / PACK, bl = i % PACK;
    const int b = g * PACK + bl, c = c0 + cc;
    if (b < B && c <= e) packed[packed_at(B, e, c, b)] = tile[cc][bl];
}

// One tile of rows e = E*QROWS .. E*QROWS + QROWS - 1 (FULL: all of them below C) for one lane and QDAYS days.
//   sd[k]   the basin group's first element of day k in column 0 (column c is c * stride further)
//   packed  the basin group's first element of the packed factor (packed row i is i * B further)
//   lane    the lane's basin inside the group, 0..63: the only per-lane part of an address
// A row e takes the columns 0..e in ascending order: first the columns every row of the tile has (0..E*QROWS), then
// the tile's own triangle.  Elements with c > e are never addressed.  The first loop is written as a rotation: the operands
// of column c + 1 are fetched before column c is used (the last turn fetches its own column again: an address that is
// valid anyway).  hipcc folds the rotation back -- a turn's loads and uses end up in the same turn -- but the form is not
// idle: it compiles to 167 VGPRs, three waves per SIMD and one counted wait per factor row, where the plain load-then-use
// loop takes 177 VGPRs and runs two waves per SIMD (profiles/r13_predictive_variance.md).
template <bool FULL>
HBVX_QF_HD void tile_rows(int B, int C, int E, const float *const (&sd)[QDAYS], int64_t stride, const float *packed,
                          unsigned lane, float (&q)[QDAYS])
{
    const int e0 = E * QROWS;
    const int nr = FULL ? QROWS : C - e0;
    const float *pm[QROWS];                     // packed row of (e, 0)
#pragma unroll
    for (int r = 0; r < QROWS; r++) pm[r] = packed + tri(e0 + (FULL || r < nr ? r : 0)) * B;
    float y[QROWS][QDAYS];
#pragma unroll
    for (int r = 0; r < QROWS; r++)
#pragma unroll
        for (int k = 0; k < QDAYS; k++) y[r][k] = 0.0f;
    int64_t so = 0, mo = 0;                     // offsets of the column in flight: in a series, in a packed row
    float sv[QDAYS], mv[QROWS], sn[QDAYS], mn[QROWS];
#pragma unroll
    for (int k = 0; k < QDAYS; k++) sn[k] = (sd[k] + so)[lane];
#pragma unroll
    for (int r = 0; r < QROWS; r++) mn[r] = (pm[r] + mo)[lane];
    for (int c = 0; c <= e0; c++) {
#pragma unroll
        for (int k = 0; k < QDAYS; k++) sv[k] = sn[k];
#pragma unroll
        for (int r = 0; r < QROWS; r++) mv[r] = mn[r];
        if (c < e0) { so += stride; mo += B; }
#pragma unroll
        for (int k = 0; k < QDAYS; k++) sn[k] = (sd[k] + so)[lane];
#pragma unroll
        for (int r = 0; r < QROWS; r++) mn[r] = (pm[r] + mo)[lane];
#pragma unroll
        for (int r = 0; r < QROWS; r++)
            if (FULL || r < nr) {
#pragma unroll
                for (int k = 0; k < QDAYS; k++) y[r][k] = __builtin_fmaf(mv[r], sv[k], y[r][k]);
            }
    }
#pragma unroll
    for (int j = 1; j < QROWS; j++) {
        if (!FULL && j >= nr) break;
        so += stride; mo += B;
#pragma unroll
        for (int k = 0; k < QDAYS; k++) sv[k] = (sd[k] + so)[lane];
#pragma unroll
        for (int r = j; r < QROWS; r++)
            if (FULL || r < nr) {
                const float m1 = (pm[r] + mo)[lane];
#pragma unroll
                for (int k = 0; k < QDAYS; k++) y[r][k] = __builtin_fmaf(m1, sv[k], y[r][k]);
            }
    }
#pragma unroll
    for (int r = 0; r < QROWS; r++)
        if (FULL || r < nr) {
#pragma unroll
            for (int k = 0; k < QDAYS; k++) q[k] = __builtin_fmaf(y[r][k], y[r][k], q[k]);
        }
}

// One lane: basin b0 + lane of the group that starts at basin b0, days t0 .. t0 + QDAYS - 1 (those below T are
// stored).  A tail lane passes the group's last basin and store = false; a day past T is computed on day T - 1 and
// not stored.
HBVX_QF_HD void lane_days(int T, int B, int C, const float *s, int64_t stride, const float *packed, int t0, int b0,
                          unsigned lane, bool store, float *q_out)
{
    const float *sd[QDAYS];
#pragma unroll
    for (int k = 0; k < QDAYS; k++) sd[k] = s + (int64_t)(t0 + k < T ? t0 + k : T - 1) * B + b0;
    float q[QDAYS];
#pragma unroll
    for (int k = 0; k < QDAYS; k++) q[k] = 0.0f;
    const int NF = C / QROWS;                   // full tiles
    for (int E = 0; E < NF; E++) tile_rows<true>(B, C, E, sd, stride, packed + b0, lane, q);
    if (NF * QROWS < C) tile_rows<false>(B, C, NF, sd, stride, packed + b0, lane, q);
    if (!store) return;
#pragma unroll
    for (int k = 0; k < QDAYS; k++)
        if (t0 + k < T) (q_out + (int64_t)(t0 + k) * B + b0)[lane] = q[k];
}

} // namespace hbvx_qfk
