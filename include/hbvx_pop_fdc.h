/* hbvx_pop_fdc.h -- C ABI of the population flow-duration call of the explicit models (HBV 1.0 / 1.1p / 2.0): for P
 * candidate parameter sets per basin, hbvx_population_stats' four chains and, from the same launch, the simulated
 * flow-duration curve sampled at K per-basin thresholds -- exceedance counts and the volume above each threshold.
 * Exported by the same shared library as include/hbvx.h; additive to its ABI version (HBVX_ABI_VERSION is unchanged, the
 * struct below carries an abi_version of its own).  Device pointers, float32 / int32, the caller's stream.
 *
 * The thresholds are the caller's, fixed on the observed side (the observed flows exceeded with given probabilities, a
 * flood stage), so nothing is sorted: with y the routed ensemble-mean flow of candidate c in basin b on day t -- the
 * value hbvx_population_stats transforms and scores, and stores in `sim` -- a day ENTERS when t >= t_first and its
 * weight flow.pop.w[t - t_first][b] is > 0 (w NULL: every such day enters; the weight is a mask, it scales nothing), and
 * for every k in 0..K-1, over the entering days in ascending order,
 *     y > thr[k][b]:    count[c][k][b] += 1        volume[c][k][b] = volume[c][k][b] + y      (float32, from 0)
 * The comparison is on y itself under every transform (a monotone transform does not move an exceedance count); a day
 * at the threshold is not above it, a NaN flow is above nothing.
 *
 * Guarantees: (1) flow.pop.cost, flow.s1 / s2 / s3 and flow.pop.sim have the bits hbvx_population_stats gives on the
 * same arguments; (2) count[c][k][b] and volume[c][k][b] depend on candidate c's values and thr[k][b] alone -- not on
 * K, the order of the thresholds, n_cand, the other candidates or sim; (3) no atomics, every sum runs in day order, two
 * calls agree bit for bit; (4) every element of count and volume is written; (5) argument errors are reported before
 * anything is launched.
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text:
 * hbvx_population_stats', and HBVX_E_NULL (pf, thr, count, volume), HBVX_E_ABI (pf->abi_version), HBVX_E_SHAPE (n_thr
 * outside 1..HBVX_POP_FDC_MAX_THR), HBVX_E_UNSUPPORTED (HBVX_MODEL_HBVADJ, HBVX_MODEL_HOURLY). */
#ifndef HBVX_POP_FDC_H
#define HBVX_POP_FDC_H
#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_POP_FDC_ABI_VERSION 1
#define HBVX_POP_FDC_MAX_THR 32

typedef struct hbvx_pop_fdc {
    int32_t abi_version;           /* HBVX_POP_FDC_ABI_VERSION */
    int32_t n_thr;                 /* K, 1..HBVX_POP_FDC_MAX_THR */
    hbvx_pop_stats flow;           /* hbvx_population_stats' arguments */
    const float *thr;              /* [K,B] thresholds in the units of the flow, any order */
    int32_t *count;                /* [P,K,B] entering days with y > thr */
    float *volume;                 /* [P,K,B] the sum of y over those days */
} hbvx_pop_fdc;

/* sizeof of the struct above as the library was built: 0 hbvx_pop_fdc; 0 for any other index. */
uint64_t hbvx_pop_fdc_sizeof(int which);

int hbvx_population_fdc(const hbvx_desc *d, const hbvx_pop_fdc *pf, void *stream);

#ifdef __cplusplus
}
#endif
#endif
