/* hbvx_pop_events.h -- C ABI of the population flood-event call of the explicit daily models (HBV 1.0 / 1.1p / 2.0): for
 * P candidate parameter sets per basin, hbvx_population_stats' four chains and, from the same launch, the peak, the day
 * of the peak and the volume of every candidate's routed flow inside E per-basin event windows.  Exported by the same
 * shared library as include/hbvx.h; additive to its ABI version (HBVX_ABI_VERSION is unchanged, the struct below carries
 * an abi_version of its own).  Device pointers, float32 / int32, the caller's stream.
 *
 * The windows are the caller's, fixed on the observed side (the E highest separated floods of the observed record), in
 * SCORED days: day rel = t - t_first of the call, 0 .. T_out - 1 with T_out = T - t_first.  With y the routed
 * ensemble-mean flow of candidate c in basin b on a day -- the value hbvx_population_stats transforms and scores, and
 * stores in `sim`; y itself under every transform -- a window [s, f] takes the days s .. f in ascending order:
 *     y > peak:  peak = y, peak_day = rel          volume = volume + y      (float32, from -inf, -1, +0)
 * A plateau keeps its first day; a NaN flow is above nothing (it leaves peak and peak_day alone and poisons volume); -0
 * is not above +0.  Weights do not enter: the window is the mask.
 *
 * The cursor rule.  A basin's rows are walked once, in order e = 0 .. E-1, with last = -1.  With
 * f = min(end[e][b], T_out - 1), row e is LIVE iff start[e][b] > last and f >= start[e][b]; a live row takes the days
 * start[e][b] .. f and sets last = f.  Any other row is ABSENT and holds -inf, -1, +0: start < 0, end < start, and a row
 * that overlaps or is not ahead of the previous live one.  So any content of start / end is safe: no day outside
 * 0 .. T_out - 1 is touched, nothing outside row e of the three outputs is written for row e, and a lane takes at most E
 * cursor steps.  On well-formed windows (a basin's windows strictly ascending and disjoint in its first rows, (-1, -1) in
 * the rows it does not fill) every present row is live, and a slot has the bits hbvx_gage_population_events
 * (include/hbvx_gage_events.h) gives on the call's own `sim` with the same windows.
 *
 * Guarantees: (1) flow.pop.cost, flow.s1 / s2 / s3 and flow.pop.sim have the bits hbvx_population_stats gives on the
 * same arguments; (2) peak / peak_day / volume [c][e][b] depend on candidate c's values and on basin b's windows up to
 * row e alone -- not on n_events, the rows after e, n_cand, the other candidates, the other basins or sim; (3) no
 * atomics, every sum runs in day order, two calls agree bit for bit; (4) every element of the three outputs is written;
 * (5) argument errors are reported before anything is launched.
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text:
 * hbvx_population_stats', and HBVX_E_NULL (pe, start, end, peak, peak_day, volume), HBVX_E_ABI (pe->abi_version),
 * HBVX_E_SHAPE (n_events outside 1 .. T - t_first, or n_events * B above 2^30: a row is addressed with 32 bits),
 * HBVX_E_UNSUPPORTED (HBVX_MODEL_HBVADJ, HBVX_MODEL_HOURLY). */
#ifndef HBVX_POP_EVENTS_H
#define HBVX_POP_EVENTS_H
#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_POP_EVENTS_ABI_VERSION 1

typedef struct hbvx_pop_events {
    int32_t abi_version;           /* HBVX_POP_EVENTS_ABI_VERSION */
    int32_t n_events;              /* E, 1 .. T - t_first, E * B <= 2^30 */
    hbvx_pop_stats flow;           /* hbvx_population_stats' arguments */
    const int32_t *start;          /* [E,B] first scored day of the window, inclusive */
    const int32_t *end;            /* [E,B] last scored day of the window, inclusive; clamped to T - t_first - 1 */
    float *peak;                   /* [P,E,B] the highest y of the window */
    int32_t *peak_day;             /* [P,E,B] the FIRST scored day at that flow; -1: absent, or no y above -inf */
    float *volume;                 /* [P,E,B] the float32 sum of the window's y in day order */
} hbvx_pop_events;

/* sizeof of the struct above as the library was built: 0 hbvx_pop_events; 0 for any other index. */
uint64_t hbvx_pop_events_sizeof(int which);

int hbvx_population_events(const hbvx_desc *d, const hbvx_pop_events *pe, void *stream);

#ifdef __cplusplus
}
#endif
#endif
