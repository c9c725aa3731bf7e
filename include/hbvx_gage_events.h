/* hbvx_gage_events.h -- C ABI of the flood-event statistics of the hourly model's population evaluation: per
 * (candidate, event, gage) the peak of the hourly gage series inside an event window, the hour of that peak and the
 * volume of the window.  The windows are fixed on the OBSERVED side (per gage, by the caller), so nothing is detected on
 * the simulated series: a max, a first-argmax and an ordered sum over a few dozen hours of the [P,T,G] series that
 * hbvx_gage_population_stats (include/hbvx_gage_pop.h) writes with gp->series.  No series leaves the device.
 * Exported by the same shared library as include/hbvx.h; additive to its ABI version (HBVX_ABI_VERSION is unchanged, the
 * struct below carries an abi_version of its own).  Device pointers, the caller's stream.
 *
 * One (candidate c, event e, gage g), with s = start[e][g] and f = min(end[e][g], T - 1):
 *     peak = -inf     hour = -1     vol = +0.0f
 *     for t = s .. f, ascending, y = series[c][t][g]:
 *         if (y > peak) { peak = y; hour = t; }
 *         vol = vol + y                               (one float32 addition per hour)
 *     peak[c][e][g] = peak     peak_hour[c][e][g] = hour     volume[c][e][g] = vol
 * so that
 *   - a plateau keeps its FIRST hour;
 *   - a NaN flow is above nothing: it leaves peak and hour alone (a window of NaNs alone gives -inf, -1) and poisons vol;
 *   - -0 is not above +0.
 * Absent and malformed windows: the call is safe for ANY content of start / end and reads no hour outside 0 .. T-1.
 * start < 0 or end < start (after the clamp of end to T - 1, so a start >= T too) is an absent slot: -inf, -1, +0 are
 * stored.  Every slot of [P,E,G] is written; the outputs need no fill.
 * No atomics; two calls agree bit for bit; a slot's bits depend on its candidate's series and its own window alone -- not
 * on E, the other events or gages, the order of the events, or n_cand.
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise, hbvx_last_error() has the text; every argument
 * error is reported before anything is launched. */
#ifndef HBVX_GAGE_EVENTS_H
#define HBVX_GAGE_EVENTS_H
#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_GAGE_EVENTS_ABI_VERSION 1

typedef struct hbvx_gage_events {
    int32_t abi_version;           /* HBVX_GAGE_EVENTS_ABI_VERSION */
    int32_t n_cand;                /* P, 1..65535 */
    int32_t T, G;                  /* hours and gages of the series, >= 1 */
    int32_t n_events;              /* E, 1..T */
    const float *series;           /* [P,T,G] hbvx_gage_population_stats' hourly gage series */
    const int32_t *start, *end;    /* [E,G] inclusive hours, 0-based; start < 0: no such event */
    float *peak;                   /* [P,E,G] */
    int32_t *peak_hour;            /* [P,E,G] */
    float *volume;                 /* [P,E,G] */
} hbvx_gage_events;

/* Errors: HBVX_E_NULL (ev, series, start, end, peak, peak_hour, volume), HBVX_E_ABI, HBVX_E_SHAPE (n_cand outside
 * 1..65535; T or G < 1; n_events outside 1..T). */
int hbvx_gage_population_events(const hbvx_gage_events *ev, void *stream);

/* sizeof of the struct above as the library was built: 0 hbvx_gage_events; 0 for any other index. */
uint64_t hbvx_gage_events_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
