/* hbvx_gage_pop.h -- C ABI of the population evaluation of the hourly model (HBVX_MODEL_HOURLY): the scores of P
 * candidate parameter sets at the GAGES, from two calls that write no per-pair series.
 * Exported by the same shared library as include/hbvx.h; additive to its ABI version (HBVX_ABI_VERSION is unchanged, the
 * two structs below carry an abi_version of their own).  Device pointers, float32, the caller's stream.
 *
 * The hourly model's output is gage streamflow, and gages couple the units: a unit has no score.  So the call has two
 * stages and one intermediate series.
 *
 *   (1) hbvx_hourly_population_runoff   every candidate's hourly unit runoff [P,T,U]: the recurrence hbvx_forward runs
 *       on `d`, candidate c's static values standing in for the descriptor's, the hour's ensemble mean of Q (muwts
 *       honoured, 1 / M otherwise) times (float)(1.0 / 24.0) -- the module's Qs.
 *   (2) hbvx_gage_population_stats      routes every candidate's runoff to the gages and scores it there:
 *       unit hydrographs   with `dp` given, candidate c's taps of pair p from dp[c][p][0..2] by hbvx_gage_route_forward's
 *                          own arithmetic (normalised gamma taps, the fractional lag); otherwise `uh` [NPAIR,L], the taps
 *                          a forward call stored, serve every candidate;
 *       gage series        out[c][t][g] = (sum over the pairs of gage g, in CSR order, of
 *                          sum_k uh[c][p][k] * runoff[c][t-k][unit(p)] * areas[unit(p)]) / denom[g], the taps ascending
 *                          from 0, each product rounded, then the sum: hbvx_gage_route_forward's operations in its order,
 *                          so the series has that call's bits on the same runoff and parameters.  No [P,NPAIR,T] buffer
 *                          exists: a workgroup owns (1024-hour tile, gage, candidate) and adds the pairs as it goes;
 *       period means       with K periods closing at hours period_end[0] < ... < period_end[K-1]: the hours of a period
 *                          are added in ascending order, the first one assigns, one division by the hour count at the
 *                          close (a one-hour period keeps its bits); hours after the last closing hour are not scored;
 *       the four chains    per (candidate, gage), over ascending periods, on v' = v | sqrtf(v) | logf(v + eps[g]) of the
 *                          period mean v against target[k][g] (ALREADY transformed), weight w[k][g] (NULL: 1) and
 *                          shift[g]:  r = v' - o, d = v' - m, e = o - m,
 *                            sse = fmaf(w r, r, sse)   s1 = fmaf(w, d, s1)   s2 = fmaf(w d, d, s2)   s3 = fmaf(w d, e, s3)
 *                          (w r and w d rounded once): hbvx_population_stats' chains, lanes being gages.
 * No atomics; every sum runs in a fixed order; two calls agree bit for bit, and candidate c's numbers depend on c's
 * values alone (not on n_cand, the other candidates, sim or series).
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text; every argument
 * error is reported before anything is launched. */
#ifndef HBVX_GAGE_POP_H
#define HBVX_GAGE_POP_H
#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_GAGE_POP_ABI_VERSION 1

typedef struct hbvx_pop_runoff {
    int32_t abi_version;           /* HBVX_GAGE_POP_ABI_VERSION */
    int32_t n_cand;                /* P, 1..65535 */
    hbvx_pop_src p[HBVX_MAX_PARAM]; /* candidate c's static value of slot i; sta NULL: the descriptor's */
    float *runoff;                 /* [P,T,B] */
} hbvx_pop_runoff;

typedef struct hbvx_gage_pop {
    int32_t abi_version;           /* HBVX_GAGE_POP_ABI_VERSION */
    int32_t n_cand;                /* P, 1..65535 */
    const float *runoff;           /* candidate c's [T,U] runoff at runoff + c * runoff_c_stride */
    int64_t runoff_c_stride;       /* elements; 0: one runoff serves every candidate */
    const float *dp;               /* [P,NPAIR,3] unit-interval route_a, route_b, route_tau per pair, or NULL */
    const float *uh;               /* [NPAIR,L] taps of a forward call; read when dp is NULL */
    int32_t transform;             /* HBVX_POP_T_* */
    int32_t n_periods;             /* K, 1..T */
    const int32_t *period_end;     /* [K] closing hours, ascending, 0-based */
    const float *target;           /* [K,G] transformed */
    const float *w;                /* [K,G] or NULL */
    const float *shift;            /* [G] */
    const float *eps;              /* [G], read with HBVX_POP_T_LOG only */
    float *sse, *s1, *s2, *s3;     /* [P,G] each */
    float *sim;                    /* [P,K,G] the period means (not their transform), or NULL */
    float *series;                 /* [P,T,G] the hourly gage series, or NULL (it then lives in the workspace) */
} hbvx_gage_pop;

/* HBVX_MODEL_HOURLY only (any other: HBVX_E_UNSUPPORTED).  Errors: HBVX_E_NULL (d, pr, runoff), HBVX_E_ABI,
 * HBVX_E_SHAPE (n_cand outside 1..65535, candidate values for a slot the model lacks). */
int hbvx_hourly_population_runoff(const hbvx_desc *d, const hbvx_pop_runoff *pr, void *stream);

/* Scratch of hbvx_gage_population_stats for (r, gp) in bytes (caller-owned, contents undefined afterwards): the
 * unit-major runoff [P or 1,U,T], the candidates' taps [P,NPAIR,L] with dp, the gage series [P,T,G] without
 * gp->series.  0 for arguments the call would refuse. */
uint64_t hbvx_gage_population_workspace_bytes(const hbvx_gage_desc *r, const hbvx_gage_pop *gp);

/* `r` as hbvx_gage_route_forward takes it (r->dp is not read).  Errors: that call's, and HBVX_E_NULL (gp, runoff, uh
 * without dp, period_end, target, shift, sse, s1, s2, s3, eps under HBVX_POP_T_LOG, a missing or too small
 * workspace), HBVX_E_ABI, HBVX_E_SHAPE (n_cand outside 1..65535, n_periods outside 1..T, a negative stride),
 * HBVX_E_UNSUPPORTED (a transform other than the three). */
int hbvx_gage_population_stats(const hbvx_gage_desc *r, const hbvx_gage_pop *gp, void *workspace,
                               uint64_t workspace_bytes, void *stream);

/* sizeof of the structs above as the library was built: 0 hbvx_pop_runoff, 1 hbvx_gage_pop; 0 for any other index. */
uint64_t hbvx_gage_pop_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
