/* hbvx_gage_fdc.h -- C ABI of the flow-duration statistics of the hourly model's population evaluation, on the hourly
 * gage series [P,T,G] that hbvx_gage_population_stats (include/hbvx_gage_pop.h) writes with gp->series: per (candidate,
 * level, gage)
 *   hbvx_gage_population_fdc        how many scored hours lie above a threshold fixed on the observed side, and the volume
 *                                   above it (include/hbvx_pop_fdc.h's rule on the gage series: nothing is sorted);
 *   hbvx_gage_population_quantiles  the candidate's OWN flow-duration curve at given ranks: the scored hours of a
 *                                   (candidate, gage) column sorted descending on the device, and the flows at K indices.
 * No series leaves the device.  Exported by the same shared library as include/hbvx.h; additive to its ABI version
 * (HBVX_ABI_VERSION is unchanged, the struct below carries an abi_version of its own).  Device pointers, the caller's
 * stream.  One struct serves both exports; each reads the fields its prototype names and ignores the rest.
 *
 * An hour t ENTERS at gage g when scored[t][g] != 0 (the mask is the caller's: a finite observation, a weight > 0).
 *
 * hbvx_gage_population_fdc, one (candidate c, level k, gage g):
 *     n = 0     vol = +0.0f
 *     for t = 0 .. T-1, ascending, where scored[t][g] != 0, y = series[c][t][g]:
 *         if (y > thr[k][g]) { n = n + 1;  vol = vol + y; }       (one float32 addition per hour)
 *     count[c][k][g] = n     volume[c][k][g] = vol
 * so that an hour AT the threshold is not above it, a NaN flow is above nothing and -0 is not above +0.  Every slot of
 * [P,K,G] of both outputs is written; a slot's bits depend on its candidate's series, its gage's mask and its own
 * threshold alone -- not on K, the order of the levels, n_cand or the other gages.  T has no limit beyond int32.
 *
 * hbvx_gage_population_quantiles, one (candidate c, gage g):
 *     v = the n flows series[c][t][g] of the hours with scored[t][g] != 0
 *     any of them NaN:  quantile[c][k][g] = NaN for every k
 *     else sort v descending under float32's total order on non-NaN values (in which -0 sorts below +0), and
 *         quantile[c][k][g] = v[rank[k][g]]   where 0 <= rank[k][g] <= n - 1,     NaN otherwise
 * so that every rank at a gage without a scored hour gives NaN.  A sort does no arithmetic: a quantile that is not NaN
 * is a value of the series, bit for bit; the NaN stored is the quiet NaN 0x7FC00000.  Every slot of [P,K,G] is written.
 * Limit: T <= HBVX_GAGE_QUANT_MAX_T (the column padded to a power of two is then 64 KB of LDS).
 * workspace: hbvx_gage_quantiles_workspace_bytes(n_cand, T, G) bytes of device memory (the columns gage-major, as
 * sortable keys); its content before the call does not matter and nothing of it needs to outlive the call.
 *
 * No atomics; two calls agree bit for bit.
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text; every argument
 * error is reported before anything is launched. */
#ifndef HBVX_GAGE_FDC_H
#define HBVX_GAGE_FDC_H
#include "hbvx.h"
#include "hbvx_pop_fdc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_GAGE_FDC_ABI_VERSION 1
#define HBVX_GAGE_FDC_MAX_LEV HBVX_POP_FDC_MAX_THR
#define HBVX_GAGE_QUANT_MAX_T 16384

typedef struct hbvx_gage_fdc {
    int32_t abi_version;           /* HBVX_GAGE_FDC_ABI_VERSION */
    int32_t n_cand;                /* P, 1..65535 */
    int32_t T, G;                  /* hours and gages of the series, >= 1 */
    int32_t n_lev;                 /* K, 1..HBVX_GAGE_FDC_MAX_LEV */
    const float *series;           /* [P,T,G] hbvx_gage_population_stats' hourly gage series */
    const uint8_t *scored;         /* [T,G] non-zero: the hour enters */
    const float *thr;              /* [K,G] thresholds in the units of the flow, any order      (fdc) */
    int32_t *count;                /* [P,K,G] entering hours with y > thr                        (fdc) */
    float *volume;                 /* [P,K,G] the sum of y over those hours                      (fdc) */
    const int32_t *rank;           /* [K,G] 0-based indices into the descending column           (quantiles) */
    float *quantile;               /* [P,K,G]                                                    (quantiles) */
} hbvx_gage_fdc;

/* Errors: HBVX_E_NULL (gf, series, scored, thr, count, volume), HBVX_E_ABI, HBVX_E_SHAPE (n_cand outside 1..65535; T or
 * G < 1; n_lev outside 1..HBVX_GAGE_FDC_MAX_LEV; a G at which one candidate alone would need 2^32 threads, 2^30 gages). */
int hbvx_gage_population_fdc(const hbvx_gage_fdc *gf, void *stream);

/* Errors: HBVX_E_NULL (gf, series, scored, rank, quantile; workspace, or workspace_bytes below what the function under
 * it returns), HBVX_E_ABI, HBVX_E_SHAPE (as above; here from G x T = 2^24 x 2^8 on), HBVX_E_UNSUPPORTED
 * (T > HBVX_GAGE_QUANT_MAX_T). */
int hbvx_gage_population_quantiles(const hbvx_gage_fdc *gf, float *workspace, uint64_t workspace_bytes, void *stream);

/* Bytes of workspace of hbvx_gage_population_quantiles; 0 for arguments it refuses. */
uint64_t hbvx_gage_quantiles_workspace_bytes(int32_t n_cand, int32_t T, int32_t G);

/* sizeof of the struct above as the library was built: 0 hbvx_gage_fdc; 0 for any other index. */
uint64_t hbvx_gage_fdc_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
