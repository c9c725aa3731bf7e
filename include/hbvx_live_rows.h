/*
 * hbvx_live_rows.h -- an optional export of libhbvx.so beside include/hbvx.h (same ABI version; a library may lack it,
 * the CPU restatement under oracle/ does): the adjoint with a gradient buffer of the runoff series of fewer than four
 * rows.
 *
 * hbvx_bwd_io.grad_flux4 is [4,T,B]: the extra gradient of Qsim, Q0, Q1, Q2.  At the usual loss -- routed streamflow
 * only -- routing fills row 0 and the other three are zero: 59 MB at 671 basins x 7 300 days that the routing adjoint
 * wrote and the adjoint read back on every lane-day.  Here the caller says how many leading rows exist; the adjoint
 * loads those and takes the others as +0.0f, so every result keeps its bits.
 */
#ifndef HBVX_LIVE_ROWS_H
#define HBVX_LIVE_ROWS_H

#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hbvx_backward with io->grad_flux4 [n_live4,T,B], 1 <= n_live4 <= 4 (else HBVX_E_SHAPE): rows n_live4 .. 3 are never
 * read and count as zero.  n_live4 == 4 is hbvx_backward.  With fewer rows only the one-pass static adjoint of HBV 1.0
 * (row trajectory, no grad_flux) takes the call; any other call returns HBVX_E_UNSUPPORTED before anything is launched,
 * and the caller clears the dead rows of a [4,T,B] buffer and calls hbvx_backward instead.  Everything else as
 * hbvx_backward. */
int hbvx_backward_live(const hbvx_desc *d, const hbvx_bwd_io *io, int32_t n_live4, void *stream);

#ifdef __cplusplus
}
#endif

#endif
