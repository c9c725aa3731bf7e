/*
 * hbvx_route_rows.h -- an optional export of libhbvx.so beside include/hbvx.h (same ABI version; a library may lack it,
 * the CPU restatement under oracle/ does): the routing adjoint into a gradient buffer of more rows than series.
 *
 * The adjoint of the explicit models takes the gradient of its four runoff series as one [4,T,B] buffer
 * (hbvx_bwd_io.grad_flux4), of which routing fills the rows that carry a routed gradient -- one, at the usual
 * streamflow loss.  The other rows must be zero.  hbvx_route_backward writes its S rows only, so a caller had to clear
 * the rest in a launch of its own (59 MB at 671 basins x 7 300 days); here the routing adjoint's workgroups write those
 * zeros for their own days and basins, beside their arithmetic.
 */
#ifndef HBVX_ROUTE_ROWS_H
#define HBVX_ROUTE_ROWS_H

#include "hbvx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hbvx_route_backward with grad_q [grad_q_rows,T,B], grad_q_rows >= r->S: rows 0 .. S-1 are what hbvx_route_backward
 * writes, bit for bit, as are grad_ra / grad_rb and the workspace; rows S .. grad_q_rows-1 are overwritten with zeros.
 * grad_q_rows < S: HBVX_E_SHAPE.  Everything else as hbvx_route_backward. */
int hbvx_route_backward_rows(const hbvx_route_desc *r, const float *q, const float *uh,
                             const float *grad_q_rout, float *grad_q, int32_t grad_q_rows, float *grad_ra,
                             float *grad_rb, void *workspace, uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
