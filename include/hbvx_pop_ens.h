/* hbvx_pop_ens.h -- C ABI of the ensemble (particle) form of the population call of the explicit models (HBV 1.0 /
 * 1.1p / 2.0): hbvx_population_stats over a WINDOW of the descriptor's days, with storages, routing history and forcing
 * noise per particle, and the storages and the history handed back, so that a record can be walked in windows and
 * resumed -- one step of a sequential Monte-Carlo filter per launch.  An element of the assimilation ensemble is a
 * PARTICLE (the `nmul` members of a basin keep the word member); particle c is candidate c of hbvx_population_stats.
 * Exported by the same shared library as include/hbvx.h; additive to its ABI version (HBVX_ABI_VERSION is unchanged;
 * hbvx_sizeof(14) is the struct below).  Device pointers, float32 / int32, the caller's stream.
 *
 * The call runs days t_begin .. t_end-1 of the descriptor `d` (0 <= t_begin < t_end <= d->T); no row of the forcings,
 * the dynamic parameters or muwts outside those days is read.  The SCORED days are those >= t0 = max(t_begin,
 * s.pop.t_first); s.pop.target, s.pop.w and s.pop.sim are WINDOW-RELATIVE, [t_end - t0, B] and [P, t_end - t0, B]: row 0
 * is day t0.  A window without a scored day (t_first >= t_end) is valid: no row of target / w / sim is read or written
 * (target may then be NULL), and the four chains come back +0 -- the days still run and move the storages and the
 * history.  route->L is min(d->T, 15), the full record's, so a one-day window still routes through 15 taps.
 *
 * Particle c of basin b starts from
 *   a = ancestor ? clamp(ancestor[c][b], 0, n_src - 1) : src_first + c           (one int32 load per lane)
 *   storages   state_in[a][k][b][j], k = 0..4 (NULL: d->state_in[k][b][j]; that NULL too: 0.001)
 *   history    hist_in[a][k][b], k = 0..13: the UN-ROUTED ensemble-mean q of day t_begin-1-k (NULL: zeros, which is
 *              what hbvx_population_stats starts from); read when the call routes only
 * and every day takes, after the forcings are read and before the day step,
 *   P = P * p_mul[c*pm_c_stride + (t-t_begin)*pm_t_stride + b]      (one float32 multiply; p_mul NULL: no operation)
 *   T = T + t_add[c*ta_c_stride + (t-t_begin)*ta_t_stride + b]      (one float32 add;      t_add NULL: no operation)
 * (a t stride of 0 is a per-particle constant; a NULL pointer is the ABSENT operation, not "times one" / "plus zero": a
 * temperature of -0.0 stays -0.0).  PET, the dynamic parameters and muwts are never perturbed.  The candidate columns
 * s.pop.p[i].sta / ra / rb stay optional per particle (joint state-parameter particles).
 * After day t_end-1 the call writes
 *   state_out[c][k][b][j]   the five storages, by hbvx_forward's state_out convention: every lane of a real (basin,
 *                           member) writes, the padding lanes of M < 2^ceil(log2 M) write nothing -- [P,5,B,M] is dense;
 *   hist_out[c][k][b]       the history with the same meaning at t_end (when the call routes).
 * Neither may overlap state_in / hist_in (a particle's ancestor may be another's output slot): the call refuses that.
 *
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) a particle's bits depend on its own inputs alone
 * -- not on n_cand, the other particles or sim == NULL; (3) with t_begin = 0, t_end = d->T and state_in, hist_in,
 * ancestor, p_mul, t_add all NULL, s.pop.cost, s.s1 / s2 / s3 and s.pop.sim have the bits hbvx_population_stats gives;
 * (4) RESUME: consecutive windows, each fed the previous call's state_out / hist_out (ancestor NULL or the identity),
 * give bit for bit the sim rows, the final state_out and the final hist_out of the same days in one window, for every
 * split, one-day windows and windows that straddle t_first included; (5) no atomics, no scratch memory; (6) argument
 * errors are reported before anything is launched.
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text:
 * hbvx_population_stats' (target NULL only when the window has a scored day), and HBVX_E_NULL (pe, state_out; hist_out
 * when routed), HBVX_E_SHAPE (t_begin / t_end outside 0 <= t_begin < t_end <= T, n_src / src_first that leave an identity
 * ancestor outside 0..n_src-1, state_out / hist_out overlapping state_in / hist_in), HBVX_E_UNSUPPORTED
 * (HBVX_MODEL_HBVADJ, HBVX_MODEL_HOURLY). */
#ifndef HBVX_POP_ENS_H
#define HBVX_POP_ENS_H
#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_POP_ENS_HIST 14       /* HBVX_UH_MAXLEN - 1: the days of history a 15-tap window carries */

typedef struct hbvx_pop_ens {
    hbvx_pop_stats s;              /* hbvx_population_stats' arguments; target / w / sim window-relative (above) */
    int32_t t_begin, t_end;        /* the window: days t_begin .. t_end-1 of the descriptor */
    int32_t n_src;                 /* particles in state_in / hist_in: what an ancestor is clamped to; 0: s.pop.n_cand */
    int32_t src_first;             /* without `ancestor`, particle c starts from source src_first + c (a launch that takes
                                      particles c0 .. of a larger ensemble passes c0) */
    const float *state_in;         /* [n_src,5,B,M] or NULL */
    float *state_out;              /* [P,5,B,M], required */
    const float *hist_in;          /* [n_src,14,B] or NULL (zeros) */
    float *hist_out;               /* [P,14,B], required when the call routes */
    const int32_t *ancestor;       /* [P,B] or NULL (the identity) */
    const float *p_mul, *t_add;    /* each NULL or addressed as above */
    int64_t pm_c_stride, pm_t_stride, ta_c_stride, ta_t_stride;
} hbvx_pop_ens;                    /* hbvx_sizeof(14) */

int hbvx_population_ensemble(const hbvx_desc *d, const hbvx_pop_ens *pe, void *stream);

#ifdef __cplusplus
}
#endif
#endif
