/*
 * hbvx.h -- C ABI of the MI355X-native HBV time-stepper (libhbvx.so).
 *
 * The reference (mhpi/hydrodl2) has no FFI of its own: its plug-in contract is
 * the Python class `Hbv(config, device).forward(x_dict, parameters)`
 * (src/hydrodl2/models/hbv/hbv.py:284-361).  This header declares the entry
 * points a binding for that path needs; each one names the reference code it
 * replaces.  Plain pointers and sizes only -- no torch types.
 *
 *   hbvx_forward         replaces the `for t in range(nsteps)` recurrence and the
 *                        ensemble mean: hbv.py:423-511, hbv_1_1p.py:422-521,
 *                        hbv_2.py:464-581, fused with the parameter prep
 *                        (sigmoid, static-row pick, dy_drop blend, de-scaling:
 *                        hbv.py:201-208,236-256, core/calc/utils.py:9-24).
 *   hbvx_backward        replaces the autograd tape of the same lines
 *                        (SURVEY.md §3.4 / §8 a11): hand-written adjoint.
 *   hbvx_route_forward   replaces uh_gamma + uh_conv on the ensemble means:
 *                        core/calc/uh_routing.py:5-57, called at hbv.py:523-538.
 *   hbvx_route_backward  replaces conv1d/lgamma/pow autograd of those lines.
 *   hbvx_forward_tangent, hbvx_route_tangent, hbvx_bfi_tangent
 *                        replace torch.autograd.forward_ad over the same lines
 *                        (forward mode: one tangent direction per call).
 *   hbvx_forward_tangent_batch, hbvx_route_tangent_batch, hbvx_bfi_tangent_batch
 *                        the same over a leading direction axis: many directions on one
 *                        primal (sensitivity series, per-basin Jacobians).
 *   hbvx_hourly_tangent_batch, hbvx_gage_route_tangent_batch
 *                        the same for the hourly model: the sub-daily recurrence and the gage routing, many
 *                        directions per call (one direction is n_dir = 1).  hbvx_forward_tangent and
 *                        hbvx_forward_tangent_batch keep refusing HBVX_MODEL_HOURLY.
 *   hbvx_adj_tangent_batch
 *                        the same for the implicit scheme: implicit-function tangents at the solved states of
 *                        hbvx_adj_forward, many directions per call.
 *   hbvx_gram            has no counterpart in the reference: the per-basin normal equations J^T W J, J^T W r and the
 *                        cost of a Gauss-Newton / Levenberg-Marquardt calibration, straight from the direction-major
 *                        series the tangent calls write.
 *   hbvx_population_cost has no counterpart either: the weighted squared error of the routed streamflow of many
 *                        candidate parameter sets per basin in one launch (random / SCE-UA / DDS-style searches).
 *
 * Ownership: the caller allocates and owns every buffer; the library keeps no
 * state between calls and allocates nothing persistent.  All device work is
 * enqueued on `stream` (a hipStream_t passed as void*); no call synchronises.
 * Errors: 0 on success, a negative HBVX_E_* otherwise; hbvx_last_error() returns
 * a thread-local message.  Nothing throws across the ABI.
 *
 * The CPU oracle (oracle/hbv_oracle.c) implements the same ABI on host memory
 * (stream ignored) so that tests can drive both with identical descriptors.
 */
#ifndef HBVX_H
#define HBVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_ABI_VERSION 10
#define HBVX_MAX_PARAM 20
#define HBVX_NSTATE 5   /* SNOWPACK, MELTWATER, SM, SUZ, SLZ  (hbv.py:61-67) */
#define HBVX_MAX_FLUX 12
#define HBVX_UH_MAXLEN 15 /* lenF (hbv.py:526, hbv_2.py:52) */

/* Parameter slots: the order of `parameter_bounds` in every variant
 * (hbv.py:88-101,124-125; hbv_1_1p.py:87-102; hbv_2.py:90-107). */
enum hbvx_param_slot {
    HBVX_P_BETA = 0, HBVX_P_FC, HBVX_P_K0, HBVX_P_K1, HBVX_P_K2, HBVX_P_LP,
    HBVX_P_PERC, HBVX_P_UZL, HBVX_P_TT, HBVX_P_CFMAX, HBVX_P_CFR, HBVX_P_CWH,
    HBVX_P_BETAET, HBVX_P_C, HBVX_P_RT, HBVX_P_AC,
    HBVX_P_F0, HBVX_P_FMIN, HBVX_P_ALPHA /* hourly Hortonian infiltration (hbv_2_hourly.py:108-114) */
};

enum hbvx_model {
    HBVX_MODEL_HBV10 = 0,  /* n_param 12, or 13 when parBETAET is present */
    HBVX_MODEL_HBV11P = 1, /* n_param 14: + parBETAET always, capillary rise */
    HBVX_MODEL_HBV20 = 2,  /* n_param 16: + elevation TT switch, lateral flow */
    HBVX_MODEL_HBVADJ = 3, /* implicit (backward-Euler) HBV, hbvx_adj_* only; n_param 12 or 13 */
    HBVX_MODEL_HOURLY = 4  /* n_param 19: HBV 2.0 in rate form with dt = 1/24 day, storage guard-rails,
                              Hortonian infiltration excess (hbv_2_hourly.py:527-675); forcings are
                              per-step depths, fluxes are rates per day */
};

/* Ensemble-mean series written by hbvx_forward, flux[k][t][b]
 * (the buffers of hbv.py:402-420 after mean(-1): hbv.py:509,575-588). */
enum hbvx_flux {
    HBVX_F_QSIM = 0, /* Q0+Q1+Q2; weighted by muwts when given (hbv.py:508-511) */
    HBVX_F_Q0, HBVX_F_Q1, HBVX_F_Q2, HBVX_F_AET, HBVX_F_SWE, HBVX_F_RECHARGE,
    HBVX_F_EXCS, HBVX_F_EVAPFACTOR, HBVX_F_TOSOIL, HBVX_F_PERC,
    HBVX_F_CAPILLARY /* 1.1p / 2.0 only */
};

enum hbvx_error {
    HBVX_OK = 0,
    HBVX_E_NULL = -1,        /* required pointer missing */
    HBVX_E_SHAPE = -2,       /* T/B/M/n_param out of range */
    HBVX_E_UNSUPPORTED = -3, /* variant / option not built */
    HBVX_E_ABI = -4,         /* abi_version mismatch */
    HBVX_E_DEVICE = -5       /* HIP runtime error (message has the hipError) */
};

/* Where one physical parameter comes from.  Values are "unit" parameters
 * u in [0,1] (after the optional sigmoid); physical value = u*(hi-lo)+lo. */
typedef struct hbvx_param_src {
    const float *dyn;     /* per-step values or NULL (static parameter):
                             (t,b,j) at dyn[t*dyn_t_stride + b*dyn_b_stride + j] */
    const float *sta;     /* static values, required: (b,j) at sta[b*sta_b_stride + j]
                             (the reference's "last row": hbv.py:242) */
    const uint8_t *drop;  /* optional [B]; 1 = basin uses the static value although
                             the parameter is dynamic (dy_drop mask, hbv.py:245-246) */
    int64_t dyn_t_stride;
    int64_t dyn_b_stride;
    int64_t sta_b_stride;
    float lo, hi;         /* bounds (parameter_bounds) */
} hbvx_param_src;

/* Where the gradient w.r.t. the *input* values (raw if raw_sigmoid, else unit)
 * goes; same addressing as hbvx_param_src.  `dyn` rows are overwritten for
 * every (t,b,j) of the call; `sta` is accumulated into (+=) after the dyn rows,
 * so both may alias the same tensor (the reference's static row T-1 lies inside
 * the dynamic tensor).  NULL pointers skip that gradient. */
typedef struct hbvx_param_grad {
    float *dyn;
    float *sta;
    int64_t dyn_t_stride;
    int64_t dyn_b_stride;
    int64_t sta_b_stride;
} hbvx_param_grad;

typedef struct hbvx_desc {
    int32_t abi_version;  /* HBVX_ABI_VERSION */
    int32_t model;        /* enum hbvx_model */
    int32_t T;            /* steps in this call */
    int32_t B;            /* basins */
    int32_t M;            /* ensemble members per basin (nmul), 1..64 */
    int32_t n_param;      /* 12, 13, 14 or 16 */
    int32_t raw_sigmoid;  /* 1: inputs are raw NN outputs, apply sigmoid first
                             (hbv.py:201); 0: inputs already in [0,1] (hbv_2.py:211) */
    int32_t ch_prcp, ch_tmean, ch_pet; /* channel of each forcing (hbv.py:388-390) */
    float nearzero;       /* hbv.py:54 */
    int32_t adj_stop;     /* hbvx_adj_* only: how a day's system G(x) = 0 is solved and who decides that the
                             iteration stops.
                             0: joint modified Newton on the five storages (hbv_adj.py:507-581), every lane
                                stops for itself.
                             1: the same, the slowest lane of the WAVEFRONT (64 lanes = 64/Mp basins x Mp
                                members) decides -- the reference's rule, one torch.max over the batch
                                (hbv_adj.py:544,546), restricted to the lanes that share a wavefront: a
                                batch-wide maximum would need a grid barrier per Newton update.
                             2: staged solve along the block lower-triangular structure of dG/dx
                                (hbv_adj.py:425-429): snow, upper zone and lower zone in closed form
                                (piecewise linear, monotone), soil moisture by scalar Newton under
                                adj_gtol / adj_max_iter, per lane.  Same acceptance test |G|_inf <= gtol;
                                the blocks of consecutive days run as a wave pipeline. */
    const float *x;       /* forcings: (t,b,c) at x[t*x_t_stride + b*x_b_stride + c] */
    int64_t x_t_stride, x_b_stride;
    const float *ac;      /* [B] HBV 2.0 `ac_all`  (hbv_2.py:345), else NULL */
    const float *elev;    /* [B] HBV 2.0 `elev_all` (hbv_2.py:346), else NULL */
    const float *muwts;   /* optional ensemble weights (t,b,j) at
                             muwts[t*mu_t_stride + b*mu_b_stride + j] (strides may be 0) */
    int64_t mu_t_stride, mu_b_stride;
    const float *state_in; /* [5,B,M] or NULL = every storage 0.001 (hbv.py:128-136);
                              hbvx_adj_*: NULL = 0 (hbv_adj.py:254) */
    hbvx_param_src p[HBVX_MAX_PARAM];
    /* hbvx_adj_* only (ignored elsewhere): Newton policy of hbv_adj.py:518-519,544 */
    float adj_gtol;        /* stop when max_i |G_i| <= gtol; reference 1e-3 */
    int32_t adj_max_iter;  /* updates allowed = max_iter + 1; reference max_iter = 3 */
} hbvx_desc;

/* Layout of the saved trajectory (hbvx_fwd_out.traj, same buffer and size either way):
 *   ROWS    traj [5,T+1,N] (storage k entering day t at traj[(k*(T+1)+t)*N + n])
 *   PACKED  traj = records [T+1,N,4] (SNOWPACK, MELTWATER, SM, SUZ) followed by SLZ rows [T+1,N].
 *           Two wide stores / loads per lane-day instead of five: what the streaming kernels for
 *           large grids use (a vector-memory instruction costs the same issue time whatever its
 *           width).  N = B*M, lane n = b*M + j.
 * `aux` (ABI <= 8: the two pre-clamp powers of every lane-day, [2,T,N] / records [T,N,2]) is no longer
 * part of the trajectory: since ABI 9 the adjoint recomputes both powers from the saved storages with
 * the forward's own instruction sequence (20 instead of 28 bytes per lane-day), and the device library
 * neither writes nor reads the pointer, in any build: there is no build switch that restores the old
 * behaviour.  Pass NULL (a checkpoint forward, HBVX_TRAJ_CKPT, refuses anything else). */
enum hbvx_traj_layout { HBVX_TRAJ_ROWS = 0, HBVX_TRAJ_PACKED = 1, HBVX_TRAJ_CKPT = 2 };
/* traj_layout = kind | (K << 8).  HBVX_TRAJ_CKPT with K in {4, 8, 16}: `traj` holds only the five
 * storages entering days 0, K, 2K, ... as [ceil(T/K), 5, N] (20/K bytes per lane-day instead of 20);
 * hbvx_backward re-materialises each K-day segment from its checkpoint (one extra
 * forward step per day).  The caller chooses it when the full trajectory does not fit
 * (100 000 basins x 16 x 7 300 days: 327 GB of trajectory against 29 GB of checkpoints at K = 8, 15 GB at
 * K = 16; the block-wise adjoint re-materialises one block of days at a time into caller scratch:
 * at most HBVX_CKPT_SCRATCH_MB (default 2048 MB) of trajectory -- or 2 K days of it, 40 K N bytes, if that
 * is more -- plus the block's gradient-series windows, two 20 N-byte carries and the inner adjoint's own
 * workspace; hbvx_ckpt_workspace_bytes returns the exact sum). */
#define HBVX_TRAJ_KIND(layout) ((layout) & 0xFF)
#define HBVX_TRAJ_CKPT_DAYS(layout) ((layout) >> 8)

typedef struct hbvx_fwd_out {
    float *flux;      /* [n_flux,T,B] or NULL (state warm-up: hbv.py:557-559) */
    float *state_out; /* [5,B,M] storages after the last step, required */
    float *traj;      /* optional [5,T+1,B*M]: storages entering step t; row T = final.
                         Needed by hbvx_backward; rows 1..T are HBV 2.0's state series
                         (hbv_2.py:571-575) */
    float *aux;       /* unused since ABI 9 (see above): NULL */
    int32_t n_flux;   /* 11 (HBV 1.0) or 12 */
    int32_t traj_layout; /* enum hbvx_traj_layout: how traj / aux are laid out.  Must be what
                            hbvx_preferred_traj_layout() returns for this desc, or HBVX_TRAJ_ROWS */
    void *zero_ptr;      /* ABI 10, optional: a caller-owned buffer (16-byte aligned) the caller needs ZEROED later -- its
                            dense gradient tensor ([T,B,ny]: 3.8 GB at config 2).  The pipelined forward is a latency
                            chain on 168 of 256 CUs; surplus workgroups of the SAME launch, on the CUs it leaves idle,
                            write zeros into this buffer in 256 KB pieces, front to back, for as long as the recurrence
                            runs, and stop with it (same stream, same launch: no cross-stream ownership of the buffer,
                            and the forward is never longer than its recurrence).  How many pieces they wrote is left in
                            zero_state[0]; hbvx_zero_rest() then fills what is missing -- all of it when another
                            kernel family took the call (zero_state[0] stays 0).  NULL: nothing.  The CPU oracle
                            leaves everything to hbvx_zero_rest. */
    uint64_t zero_bytes; /* multiple of 16 */
    void *zero_state;    /* device memory, two uint32 words, ZERO on entry ([0]: pieces claimed, [1]: workgroups of the
                            recurrence that have finished); required with zero_ptr */
} hbvx_fwd_out;

typedef struct hbvx_bwd_io {
    const float *traj;       /* from hbvx_forward, required */
    const float *aux;        /* unused since ABI 9: NULL */
    const float *grad_flux;  /* [n_flux,T,B] dL/d(flux series) or NULL (= zeros) */
    const float *grad_flux4; /* optional [4,T,B]: extra gradient of series 0..3 (Qsim,Q0,Q1,Q2),
                                i.e. grad_q of hbvx_route_backward; added to grad_flux */
    const float *grad_state_out; /* optional [5,B,M]: dL/d(final storages) (adjoint seed; NULL = 0) */
    float *grad_x;           /* optional, addressed like desc->x (overwritten) */
    float *grad_muwts;       /* optional [T,B,M] contiguous (overwritten) */
    float *grad_state_in;    /* optional [5,B,M] (overwritten) */
    int32_t n_flux;
    int32_t traj_layout;     /* the layout the forward call wrote traj / aux in */
    hbvx_param_grad g[HBVX_MAX_PARAM];
    void *workspace;          /* optional caller-owned scratch of hbvx_backward_workspace_bytes();
                                 enables the time-parallel (chunked) adjoint */
    uint64_t workspace_bytes;
    void *store_gate;         /* optional hipEvent_t: `stream` waits for it before the first kernel that STORES
                                 dynamic-parameter / forcing / muwts gradients is launched (kernels that only read
                                 -- the transfer-map and scan passes of the time-parallel adjoint -- run ahead of
                                 it).  Lets the caller fill the gradient tensor ([T,B,ny]: 3.8 GB at config 2) on
                                 another stream BESIDE the first half of the adjoint instead of in front of it.
                                 NULL: no wait.  The CPU oracle ignores it. */
} hbvx_bwd_io;

/* Unit-hydrograph routing of S series that share one UH per basin. */
typedef struct hbvx_route_desc {
    int32_t abi_version;
    int32_t T, B, S;      /* steps, basins, series (4: Qsim,Q0,Q1,Q2 at hbv.py:530-538) */
    int32_t L;            /* UH length = min(T, 15) (uh_routing.py:8) */
    int32_t raw_sigmoid;  /* routing parameters are raw (hbv.py:212) or unit (hbv_2.py:228) */
    const float *ra;      /* route_a input of basin b at ra[b*r_stride] */
    const float *rb;      /* route_b input of basin b at rb[b*r_stride] */
    int64_t r_stride;
    float a_lo, a_hi, b_lo, b_hi; /* routing_parameter_bounds (hbv.py:102-105) */
} hbvx_route_desc;

int hbvx_version(void);                 /* HBVX_ABI_VERSION */
const char *hbvx_last_error(void);
const char *hbvx_backend(void);         /* "hip:gfx950" or "cpu-oracle" */
uint64_t hbvx_sizeof(int which);        /* 0 desc, 1 fwd_out, 2 bwd_io, 3 route_desc,
                                           4 param_src, 5 param_grad, 6 gage_desc, 7 tan_io, 8 tan_batch,
                                           9 gram_desc, 10 pop, 11 pop_stats, 12 pop_joint,
                                           13 pop_period, 14 pop_ens (hbvx_pop_ens.h): layout check */
/* Diagnostic: the kernel family that took the process's last hbvx_forward (direction 0) / hbvx_backward (1) call --
 * "pipe", "stream2", "stream", "tiled", "simple", "chunked", "ckpt-block:<family>", "ckpt-lds"; "oracle" in the CPU
 * restatement.  The parity tests assert that the family they mean to pin against the reference is the one that ran. */
const char *hbvx_last_dispatch(int direction);
/* 1 when the last hbvx_forward / hbvx_adj_forward of this thread carried fill workgroups for hbvx_fwd_out.zero_ptr in its
 * launch (the pipelined forward with idle CUs), else 0 (diagnostic, like hbvx_last_dispatch). */
int hbvx_zero_in_launch(void);
/* Zero what the forward's launch left of hbvx_fwd_out.zero_ptr: pieces zero_state[0] .. end (HBVX_ZERO_PIECE bytes each).
 * Asynchronous on `stream`, which must be ordered behind the forward call. */
#define HBVX_ZERO_PIECE (256u * 1024u)
int hbvx_zero_rest(void *ptr, uint64_t bytes, const void *zero_state, void *stream);

/* The trajectory layout this library wants for the problem (grid size, dynamic set): pass the
 * value in hbvx_fwd_out.traj_layout and hbvx_bwd_io.traj_layout.  HBVX_TRAJ_ROWS is always accepted. */
int hbvx_preferred_traj_layout(const hbvx_desc *d);

int hbvx_forward(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream);
int hbvx_backward(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream);
/* Scratch bytes the time-parallel adjoint wants for this problem (0: not applicable). */
uint64_t hbvx_backward_workspace_bytes(const hbvx_desc *d);
/* Scratch bytes hbvx_backward wants with HBVX_TRAJ_CKPT and interval K (hbvx_bwd_io.workspace): one
 * block of re-materialised trajectory + the block's gradient series + what the regular adjoint needs
 * for a block.  With it the adjoint runs block-wise on the fast kernels; without, a serial fallback. */
uint64_t hbvx_ckpt_workspace_bytes(const hbvx_desc *d, int32_t K);

/* q [S,T,B] -> uh [B,L] (normalised gamma UH) and q_rout [S,T,B]. */
int hbvx_route_forward(const hbvx_route_desc *r, const float *q, float *uh, float *q_rout,
                       void *stream);
/* Baseflow index (hbv.py:562-567): bfi[b] = 100 * sum_t q2[t,b] / (sum_t qs[t,b] + nearzero), with
 * qs, q2 [T,B] (routed streamflow and routed groundwater flow); fixed-order sums (deterministic). */
int hbvx_bfi(int32_t T, int32_t B, const float *qs, const float *q2, float nearzero, float *bfi,
             void *stream);

/* Scratch bytes hbvx_route_backward needs (per-time-chunk partial tap gradients). */
uint64_t hbvx_route_workspace_bytes(const hbvx_route_desc *r);
/* grad_q_rout [S,T,B] -> grad_q [S,T,B] (overwritten) and the gradient w.r.t. the
 * routing inputs, accumulated (+=) at grad_ra[b*r_stride], grad_rb[b*r_stride].
 * `workspace` is caller-owned scratch of at least hbvx_route_workspace_bytes(r). */
int hbvx_route_backward(const hbvx_route_desc *r, const float *q, const float *uh,
                        const float *grad_q_rout, float *grad_q, float *grad_ra,
                        float *grad_rb, void *workspace, uint64_t workspace_bytes,
                        void *stream);
/* hbvx_route_backward into a grad_q buffer of more rows than series, the rest zeroed in the launch: the optional export
 * hbvx_route_backward_rows, include/hbvx_route_rows.h. */

/* Gage routing of unit runoff (hbv_2_hourly.py:800-897 `distr_routing` + `_frac_shift1d`): for every
 * (gage, unit) pair with outlet_topo == 1 a normalised gamma unit hydrograph of L = min(T, 72)
 * taps (core/calc/uh_routing.py:5-22), shifted by tau = k + f as (1-f) w[t-k] + f w[t-k-1] with zero
 * padding when lag_uh; out[t,g] = sum_{pairs of g} sum_k uh[p,k] qs[t-k,unit(p)] areas[unit(p)] / denom[g].
 * With the identity topology (one pair per unit, areas = denom = 1, lag_uh = 0) this is the
 * 72-tap per-unit routing of hbv_2_hourly.py:693-700.
 * Index arrays are built by the caller from outlet_topo: pairs sorted by gage (gage_ptr: CSR over
 * gages) and, for the backward gather, the pair indices grouped by unit (unit_ptr / unit_pairs). */
#define HBVX_GAGE_MAXLEN 72
typedef struct hbvx_gage_desc {
    int32_t abi_version;
    int32_t T, U, G;           /* steps, units, gages */
    int32_t NPAIR;             /* (gage, unit) pairs */
    int32_t L;                 /* min(T, 72) */
    int32_t lag_uh;            /* apply the fractional shift by route_tau */
    int32_t reserved0;
    const int32_t *pair_unit;  /* [NPAIR] unit of each pair, pairs ordered by gage */
    const int32_t *gage_ptr;   /* [G+1] pairs of gage g: gage_ptr[g] .. gage_ptr[g+1]-1 */
    const int32_t *pair_gage;  /* [NPAIR] gage of each pair */
    const int32_t *unit_ptr;   /* [U+1] CSR over units into unit_pairs */
    const int32_t *unit_pairs; /* [NPAIR] pair indices grouped by unit */
    const float *areas;        /* [U] */
    const float *denom;        /* [G] upstream area of each gage, clamped at 1e-6 (:849) */
    const float *dp;           /* [NPAIR,3] unit-interval route_a, route_b, route_tau (contiguous) */
    float a_lo, a_hi, b_lo, b_hi, tau_lo, tau_hi; /* distr_parameter_bounds (:120-124) */
} hbvx_gage_desc;

/* Scratch for the two calls below (bytes; caller-owned, contents undefined afterwards): the
 * time-major runoff / gradient are transposed once per call so that a unit's (gage's) series is
 * contiguous when the kernels stage it. */
uint64_t hbvx_gage_route_workspace_bytes(const hbvx_gage_desc *r);
/* qs [T,U] -> uh [NPAIR,L] (the lagged unit hydrographs, kept for the backward) and out [T,G]. */
int hbvx_gage_route_forward(const hbvx_gage_desc *r, const float *qs, float *uh, float *out,
                            void *workspace, uint64_t workspace_bytes, void *stream);
/* grad_out [T,G] -> grad_qs [T,U] and grad_dp [NPAIR,3] (both overwritten). */
int hbvx_gage_route_backward(const hbvx_gage_desc *r, const float *qs, const float *uh,
                             const float *grad_out, float *grad_qs, float *grad_dp,
                             void *workspace, uint64_t workspace_bytes, void *stream);

/* Implicit HBV ("HBV adjoint", hbv_adj.py): per day solve G(x) = (x - x_t)/dt - f(x, theta_t, t) = 0
 * (hbv_adj.py:669-687) by modified Newton (hbv_adj.py:507-581) with the analytic 5x5 Jacobian;
 * flux[0][t][b] = ensemble mean of q0+q1+q2 at the solved state (hbv_adj.py:309-317).
 * Uses hbvx_desc (model HBVX_MODEL_HBVADJ; `drop` is per LANE [B*M], hbv_adj.py:182-189),
 * hbvx_fwd_out with n_flux = 1 (traj rows 1..T = solved states) and hbvx_bwd_io.
 * The backward is the implicit-function adjoint the reference intends (hbv_adj.py:617-633):
 * (dG/dx)^T lambda = dL/dx, dL/dtheta = -lambda^T dG/dtheta, dL/dx_t = lambda/dt. */
int hbvx_adj_forward(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream);
int hbvx_adj_backward(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream);

/* Forward-mode derivative (tangent-linear model) of hbvx_forward, HBV 1.0 / 1.1p / 2.0 only (the hourly model:
 * hbvx_hourly_tangent_batch below).  One direction per call:
 * given the tangents of the raw inputs, the tangents of the flux series and of the final storages.  The call re-runs
 * the primal day by day beside the five state tangents (one lane per (basin, member)); the primal outputs themselves
 * come from hbvx_forward.  hbvx_route_tangent and hbvx_bfi_tangent run the kernels of the several-direction calls
 * below with one direction; hbvx_forward_tangent runs an instantiation of its own of the several-direction kernel's
 * text (every series, no direction strides: 3 % faster than the several-direction instance at one direction) with the
 * same arithmetic.  Conventions are torch's forward formulas (binary minimum: 1/2 each at a tie; clamps
 * inclusive; d(x**y) = 0 at x == 0), the transpose of hbvx_backward's.  dy_drop masks (hbvx_param_src.drop) blend
 * the tangents as they blend the values.  Tangents of `ac` / `elev` are not supported.
 * Tangent of a raw parameter tensor: same addressing as hbvx_param_src (dyn rows for every (t,b,j) of the call
 * when the parameter is dynamic, sta for the static value); NULL = zero tangent. */
typedef struct hbvx_param_tan {
    const float *dyn;
    const float *sta;
    int64_t dyn_t_stride;
    int64_t dyn_b_stride;
    int64_t sta_b_stride;
} hbvx_param_tan;

typedef struct hbvx_tan_io {
    const float *x;          /* tangent of desc->x, addressed like it (same strides), or NULL */
    const float *muwts;      /* tangent of desc->muwts, addressed like it, or NULL */
    const float *state_in;   /* [5,B,M] tangent of desc->state_in, or NULL (= 0) */
    hbvx_param_tan p[HBVX_MAX_PARAM];
    float *tan_flux;         /* [n_flux,T,B] (overwritten) or NULL (no series: a state warm-up) */
    float *tan_state_out;    /* [5,B,M] (overwritten), required */
    int32_t n_flux;          /* 11 (HBV 1.0) or 12 */
    int32_t reserved0;
} hbvx_tan_io;

int hbvx_forward_tangent(const hbvx_desc *d, const hbvx_tan_io *io, void *stream);
/* Tangent of hbvx_route_forward: q [S,T,B] and uh [B,L] from that call, q_dot [S,T,B] (or NULL = 0) the tangent of
 * q, ra_dot / rb_dot the tangents of the routing inputs at ra_dot[b*r->r_stride] (or NULL = 0):
 * q_rout_dot = conv(q_dot, uh) + conv(q, d uh / d(a, b) . (a_dot, b_dot))  [S,T,B] (overwritten). */
int hbvx_route_tangent(const hbvx_route_desc *r, const float *q, const float *uh, const float *q_dot,
                       const float *ra_dot, const float *rb_dot, float *q_rout_dot, void *stream);
/* Tangent of hbvx_bfi: bfi_dot[b] = 100 (sum_t q2_dot / (S0 + nearzero) - sum_t q2 * sum_t qs_dot / (S0 + nearzero)^2),
 * S0 = sum_t qs; fixed-order sums. */
int hbvx_bfi_tangent(int32_t T, int32_t B, const float *qs, const float *q2, const float *qs_dot, const float *q2_dot,
                     float nearzero, float *bfi_dot, void *stream);

/* Several directions per call (optional exports; a library may lack them).  The same tangent-linear model as
 * hbvx_forward_tangent, hbvx_route_tangent and hbvx_bfi_tangent over a leading direction axis of n_dir: one launch, the
 * directions run as further workgroups beside each other on the SIMDs one direction leaves idle.  Direction d's
 * arithmetic is the one-direction call's, operation for operation.
 * Every input tangent is a base pointer plus a per-direction stride in elements (direction d at ptr + d * stride,
 * addressed within a direction like the one-direction struct); a NULL pointer or a stride of 0 means a zero tangent.
 * The static part of a parameter tangent may therefore point into a compact [n_dir,B,ny] array (sta_d_stride = B*ny,
 * sta_b_stride = ny).  The dyn rows of the parameter tangents cover days dyn_t0 .. T-1 of the call (day t at row
 * t - dyn_t0); on earlier days the dynamic tangents are zero.  dyn_t0 = 0 is a full [n_dir,T,B,ny] tensor; dyn_t0 = T-1
 * with dyn pointing into the compact array is "only the last row moves".
 * Outputs: only the series whose bit is set in flux_mask (bit k = enum hbvx_flux k, below n_flux) are computed and
 * written, in ascending order of k: tan_flux [n_dir, n_sel, T, B], n_sel = popcount(flux_mask); all twelve series of
 * 671 basins x 7300 days are 235 MB per direction, a streamflow Jacobian needs one.  tan_flux may be NULL when
 * flux_mask is 0 (a state warm-up).  tan_state_out [n_dir,5,B,M] is required. */
typedef struct hbvx_tan_batch {
    int32_t n_dir;           /* >= 1 */
    int32_t n_flux;          /* 11 (HBV 1.0) or 12: what flux_mask is checked against */
    uint32_t flux_mask;
    int32_t dyn_t0;          /* 0 .. T-1 */
    const float *x;          /* tangent of desc->x, addressed like it within a direction, or NULL */
    int64_t x_d_stride;
    const float *muwts;      /* tangent of desc->muwts, addressed like it within a direction, or NULL */
    int64_t mu_d_stride;
    const float *state_in;   /* [n_dir,5,B,M] at state_d_stride per direction, or NULL */
    int64_t state_d_stride;
    hbvx_param_tan p[HBVX_MAX_PARAM];
    int64_t dyn_d_stride[HBVX_MAX_PARAM];
    int64_t sta_d_stride[HBVX_MAX_PARAM];
    float *tan_flux;
    float *tan_state_out;
} hbvx_tan_batch;            /* hbvx_sizeof(8) */

int hbvx_forward_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, void *stream);
/* hbvx_route_tangent over n_dir directions: q_dot direction d at q_dot + d * q_dot_d_stride ([S,T,B] within it; the
 * leading S series of a tan_flux row), ra_dot / rb_dot of direction d at ra_dot + d * r_d_stride + b * r->r_stride;
 * q_rout_dot [n_dir,S,T,B] (overwritten).  NULL or stride 0: zero tangent.  n_dir * S <= 65535. */
int hbvx_route_tangent_batch(const hbvx_route_desc *r, int32_t n_dir, const float *q, const float *uh,
                             const float *q_dot, int64_t q_dot_d_stride, const float *ra_dot, const float *rb_dot,
                             int64_t r_d_stride, float *q_rout_dot, void *stream);
/* hbvx_bfi_tangent over n_dir directions: qs_dot / q2_dot of direction d at ptr + d * dot_d_stride ([T,B] each);
 * bfi_dot [n_dir,B] (overwritten).  n_dir <= 65535. */
int hbvx_bfi_tangent_batch(int32_t T, int32_t B, int32_t n_dir, const float *qs, const float *q2, const float *qs_dot,
                           const float *q2_dot, int64_t dot_d_stride, float nearzero, float *bfi_dot, void *stream);

/* The hourly model (optional exports; a library may lack them).
 * hbvx_hourly_tangent_batch is hbvx_forward_tangent_batch for HBVX_MODEL_HOURLY (any other model:
 * HBVX_E_UNSUPPORTED): the same struct, rules and layouts, n_flux = 12, `ac` and `elev` read per basin, 19 parameters.
 * Tangents of the forcings are depths per step, like the forcings.  One direction is n_dir = 1. */
int hbvx_hourly_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, void *stream);
/* Tangent of hbvx_gage_route_forward over n_dir directions.  Routing is bilinear in (qs, uh):
 *   out_dot = Route(qs_dot; uh) + Route(qs; uh_dot),
 * uh_dot from the closed forms of the normalised gamma taps and their fractional shift (the floor of tau contributes
 * nothing, relu's slope is 0 at 0; without lag_uh there is no tau term).  qs [T,U] and uh [NPAIR,L] are the forward
 * call's; qs_dot of direction d at qs_dot + d * qs_dot_d_stride ([T,U] within it), dp_dot at dp_dot + d *
 * dp_dot_d_stride ([NPAIR,3], unit-interval like hbvx_gage_desc.dp); NULL or a stride of 0: zero tangent, that term
 * is skipped.  out_dot [n_dir,T,G] (overwritten).  n_dir in 1..65535.  No atomics: the sum over a gage's pairs keeps
 * its fixed order, results are bit-reproducible and a direction's result does not depend on n_dir.
 * `workspace`: caller-owned scratch of at least hbvx_gage_route_tangent_workspace_bytes(r, n_dir); the directions
 * are processed in slabs so that it stays near 1 GiB however many there are. */
uint64_t hbvx_gage_route_tangent_workspace_bytes(const hbvx_gage_desc *r, int32_t n_dir);
int hbvx_gage_route_tangent_batch(const hbvx_gage_desc *r, int32_t n_dir, const float *qs, const float *uh,
                                  const float *qs_dot, int64_t qs_dot_d_stride, const float *dp_dot,
                                  int64_t dp_dot_d_stride, float *out_dot, void *workspace, uint64_t workspace_bytes,
                                  void *stream);

/* The implicit scheme (optional export; a library may lack it).
 * hbvx_adj_tangent_batch is the forward-mode derivative of hbvx_adj_forward over n_dir directions, model
 * HBVX_MODEL_HBVADJ only (any other: HBVX_E_UNSUPPORTED).  The derivative is the implicit-function one at the SOLVED
 * state: per day (I/dt - df/dx) x_dot = x_t_dot/dt + df/dtheta theta_dot + df/dclim clim_dot, evaluated at the
 * storages hbvx_adj_forward saved -- no Newton iteration is repeated, the Newton policy of the descriptor is not
 * looked at.  `traj` is the [5,T+1,B*M] trajectory (HBVX_TRAJ_ROWS) of the call being differentiated and is required.
 * hbvx_tan_batch as for hbvx_forward_tangent_batch, with n_flux = 1, flux_mask 0 or 1, muwts NULL (the scheme has no
 * ensemble weights: a non-NULL pointer is refused), state_in / tan_state_out [n_dir,5,B,M], tan_flux [n_dir,1,T,B]
 * (the ensemble mean of q0+q1+q2, member reduction and add order of hbvx_adj_forward); dyn_t0 and the per-direction
 * strides follow the rules above, `x` carries tangents of all three forcings.  Conventions are those of
 * hbvx_adj_backward (binary minimum 1/2 each at a tie, inclusive clamps, zero slope of the Tf < TT threshold), of which
 * this is the transpose.  n_dir in 1..65535; a direction's result does not depend on n_dir (bit-identical to the same
 * direction alone).  Argument errors are reported before anything is launched. */
int hbvx_adj_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, const float *traj, void *stream);

/* Per-basin normal equations (optional exports; a library may lack them).  C series that share a [T,B] grid:
 *   gram[b,c,e] = sum_t w[t,b] s[c,t,b] s[e,t,b]
 *   rhs[b,c]    = sum_t w[t,b] s[c,t,b] r[t,b]
 *   cost[b]     = sum_t w[t,b] r[t,b]^2
 * s: series c at s + c*series_stride ([T,B] contiguous inside, series_stride >= T*B): the layout the tangent kernels
 *    write, [n_dir,T,B] with the basin as the unit-stride axis, so a Jacobian's columns need no transpose.
 * w: [T,B] or NULL (= 1).  r: [T,B] or NULL (rhs and cost are then not written and may be NULL).
 * gram [B,C,C], rhs [B,C], cost [B]: overwritten completely; both triangles of gram are written.
 * workspace: caller-owned scratch of at least hbvx_gram_workspace_bytes(g), contents undefined before and after (the
 *    call does not need it cleared: every word it reads it has written).
 * Arithmetic: float32 throughout, fused multiply-adds, no atomics.  The days are cut into slices whose number and
 * length depend on (T, B) alone; a slice is summed over ascending t, the slice sums are added in ascending order.
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) gram[b,c,e] and gram[b,e,c] have the same bits
 * (only c <= e is computed, as sum_t fma(w * s_c, s_e, .), the other triangle is a copy); (3) the bits of gram[b,c,e],
 * rhs[b,c] and cost[b] do not depend on which other columns are present (C and the column tiling do not enter the
 * order of any sum).
 * Masking is the caller's job: the kernel multiplies what it is given, so w = 0 does NOT neutralise a NaN or an
 * infinity in s or r (0 * NaN = NaN).  A caller with missing observations sets both the weight and the residual of
 * those (t, b) to 0 before the call (hydrodl2_amd.normal_equations does).
 * Errors: HBVX_E_NULL (descriptor, s, gram, workspace; rhs / cost with r given), HBVX_E_SHAPE (T/B/C <= 0,
 * C > HBVX_GRAM_MAX_C, series_stride < T*B), HBVX_E_ABI. */
#define HBVX_GRAM_MAX_C 2880
typedef struct hbvx_gram_desc {
    int32_t abi_version;
    int32_t T, B, C;       /* steps, basins, series (Jacobian columns) */
    int64_t series_stride; /* elements between two series */
} hbvx_gram_desc;          /* hbvx_sizeof(9) */
uint64_t hbvx_gram_workspace_bytes(const hbvx_gram_desc *g);   /* 0 for a descriptor hbvx_gram would refuse */
int hbvx_gram(const hbvx_gram_desc *g, const float *s, const float *w, const float *r, float *gram, float *rhs,
              float *cost, void *workspace, uint64_t workspace_bytes, void *stream);

/* Per-basin quadratic form of the same series (optional exports; a library may lack them): with a lower-triangular
 * factor M_b per basin,
 *   q[t,b] = | M_b s[:,t,b] |^2 = s[:,t,b]^T (M_b^T M_b) s[:,t,b].
 * With M_b^T M_b the parameter covariance of basin b and s the Jacobian's columns this is the first-order predictive
 * variance of the series; with M_b the inverse Cholesky factor of J^T W J it is the leverage (times the weight).
 * g: hbvx_gram_desc as for hbvx_gram (T, B, C, series_stride).  s: as for hbvx_gram.
 * m: [B,C,C] row-major, lower-triangular: elements with column > row are NEVER READ and may hold anything, NaN included.
 * q: [T,B], overwritten completely.
 * workspace: caller-owned scratch of at least hbvx_quadform_workspace_bytes(g) (the lower triangles with the basin as
 *    the unit-stride axis, C(C+1)/2 * B floats), contents undefined before and after; the call does not need it cleared.
 * Arithmetic (csrc/hbv_quadform.h), float32 throughout, per (t, b):
 *   y_e = chain over ascending c = 0..e:    acc = fmaf(m[b,e,c], s[c,t,b], acc), from 0
 *   q   = chain over ascending e = 0..C-1:  q = fmaf(y_e, y_e, q), from 0
 * The factor form halves the multiply-adds of s^T Sigma s and makes the result a sum of squares.
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) q >= 0, and finite for finite inputs whose
 * result is in range; (3) the bits of q[t,b] depend on m[b] and s[:,t,b] alone -- not on T, B, the other days or
 * basins, series_stride or any tiling; (4) the upper triangle of m is not read; (5) no atomics are used.
 * Errors, reported before anything is launched: HBVX_E_NULL (descriptor, s, m, q, a missing or too small workspace),
 * HBVX_E_SHAPE (T/B/C <= 0, C > HBVX_GRAM_MAX_C, series_stride < T*B), HBVX_E_ABI. */
uint64_t hbvx_quadform_workspace_bytes(const hbvx_gram_desc *g);   /* 0 for a descriptor hbvx_quadform would refuse */
int hbvx_quadform(const hbvx_gram_desc *g, const float *s, const float *m, float *q, void *workspace,
                  uint64_t workspace_bytes, void *stream);

/* Population evaluation (optional export; a library may lack it): the cost of many candidate static-parameter sets on
 * one descriptor, one launch, nothing written but the costs.  For every candidate c and basin b the recurrence of
 * hbvx_forward runs on `d` (HBV 1.0 / 1.1p / 2.0; HBVX_MODEL_HBVADJ and HBVX_MODEL_HOURLY: HBVX_E_UNSUPPORTED) with the
 * candidate's static values in place of d->p[i].sta wherever pop->p[i].sta is set.  Dynamic parameters, drop masks,
 * muwts, state_in, ac, elev and the forcings are the descriptor's, shared by all candidates.  The ensemble mean of Q is
 * formed (with muwts) as hbvx_forward forms series HBVX_F_QSIM, routed -- when `route` is given -- through the
 * normalised gamma unit hydrograph of (c, b) with the arithmetic of hbvx_route_forward (causal, zero history before
 * day 0 of the call, taps ascending: acc += uh[k] * q[t-k]), and from day t_first on
 *   r = y - target,  cost = fmaf(w * r, r, cost)   (fmaf(r, r, cost) when w is NULL),
 * days ascending, one chain per (c, b), no atomics.  csrc/hbv_pop.h has the kernel and the per-basin arithmetic.
 * Masking is the caller's job, as for hbvx_gram: the kernel multiplies what it is given (w = 0 does not neutralise a
 * NaN in target).
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) the bits of cost[c,b] and sim[c,:,b] do not
 * depend on n_cand or on the other candidates: a candidate evaluated alone or in any subset gives the same bits;
 * (3) sim == NULL changes no bit of cost; (4) argument errors are reported before anything is launched: HBVX_E_NULL
 * (descriptor, pop, target, cost, a routing input that neither pop nor route supplies), HBVX_E_SHAPE (n_cand outside
 * 1..65535, t_first outside 0..T-1, route->L != min(T, 15), route->T / route->B unlike the descriptor's, candidate
 * values for a slot the model lacks), HBVX_E_UNSUPPORTED (model), HBVX_E_ABI.
 * Bit equality with hbvx_forward + hbvx_route_forward is not promised: the forward may be taken by another kernel
 * family. */
typedef struct hbvx_pop_src {      /* where candidate c's static value of one parameter comes from */
    const float *sta;              /* (c,b,j) at sta[c*c_stride + b*b_stride + j]; NULL: not a candidate column, */
    int64_t c_stride, b_stride;    /*   every candidate uses desc->p[i].sta                                      */
} hbvx_pop_src;

typedef struct hbvx_pop {
    int32_t n_cand;                /* P, 1..65535 */
    int32_t t_first;               /* days 0..t_first-1 of the call are simulated and enter the routing
                                      history but neither the cost nor `sim` (the module's pred_cutoff) */
    hbvx_pop_src p[HBVX_MAX_PARAM];
    const hbvx_route_desc *route;  /* NULL: cost on the un-routed ensemble mean.  Else the bounds, L, raw_sigmoid
                                      of the module's routing; ra/rb/r_stride are the NON-candidate values */
    const float *ra, *rb;          /* candidate routing inputs at ra[c*r_c_stride + b*r_b_stride]; either NULL:
                                      that one comes from route->ra / route->rb for every candidate */
    int64_t r_c_stride, r_b_stride;
    const float *target;           /* [T - t_first, B], required */
    const float *w;                /* [T - t_first, B] or NULL (= 1) */
    float *cost;                   /* [P,B], overwritten completely */
    float *sim;                    /* optional [P, T - t_first, B]: each candidate's (routed) streamflow */
} hbvx_pop;                        /* hbvx_sizeof(10) */
int hbvx_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream);

/* Population scores (optional export; a library may lack it): hbvx_population_cost with three more sums per (c, b), on
 * the raw, the square-root or the log flow, from which NSE, KGE, correlation, variability ratio and bias follow on the
 * host.  The model, the candidates, the ensemble mean, the routing, t_first and `sim` are hbvx_population_cost's: y is
 * the same number in every transform, and `sim` stores y.  Per counted day, days ascending, one chain each per (c, b),
 * no atomics, every product written here rounded once:
 *   y' = y                       (HBVX_POP_T_NONE)
 *   y' = sqrtf(y)                (HBVX_POP_T_SQRT)
 *   y' = logf(y + eps[b])        (HBVX_POP_T_LOG)
 *   r = y' - o'      d = y' - m      e = o' - m          o' = pop.target[t,b], m = shift[b]
 *   sse = fmaf(w * r, r, sse)                             -> pop.cost
 *   s1  = fmaf(w,     d, s1)
 *   s2  = fmaf(w * d, d, s2)
 *   s3  = fmaf(w * d, e, s3)                              (w = 1 when pop.w is NULL)
 * pop.target holds the target ALREADY transformed by the caller; `shift` is meant to be the weighted mean of o' (any
 * finite value is legal: the moments are about it, and the closer it lies to the mean the less they cancel).
 * Guarantees: those of hbvx_population_cost, for all four outputs; and (5) under HBVX_POP_T_NONE pop.cost has the bits
 * hbvx_population_cost gives for the same candidate, and `sim` has them under every transform.
 * Errors, before anything is launched: hbvx_population_cost's, and HBVX_E_NULL (ps, shift, s1, s2, s3; eps under
 * HBVX_POP_T_LOG), HBVX_E_UNSUPPORTED (a transform other than the three). */
enum hbvx_pop_transform { HBVX_POP_T_NONE = 0, HBVX_POP_T_SQRT = 1, HBVX_POP_T_LOG = 2 };

typedef struct hbvx_pop_stats {
    hbvx_pop pop;                  /* as above; pop.target: the TRANSFORMED target, pop.cost receives sse */
    int32_t transform;             /* HBVX_POP_T_* */
    const float *shift;            /* [B], required */
    const float *eps;              /* [B], read with HBVX_POP_T_LOG only */
    float *s1, *s2, *s3;           /* [P,B] each, overwritten completely */
} hbvx_pop_stats;                  /* hbvx_sizeof(11) */
int hbvx_population_stats(const hbvx_desc *d, const hbvx_pop_stats *ps, void *stream);

/* Population scores for a second observed series beside streamflow (optional export; a library may lack it):
 * hbvx_population_stats -- the flow term, `flow`, with exactly that call's meaning -- and in the same launch the same four
 * sums of an aux term on one un-routed flux: evapotranspiration, snow-water equivalent or a runoff component.  The aux
 * value of a day is what hbvx_forward writes for series `aux_series` of that day:
 *   v = (sum over the members of x * act) * (1 / M),   x = Q0 | Q1 | Q2 | AET | SWE of the lane's day step
 * (the plain ensemble mean: these series take 1 / M even when muwts is given), never routed and never transformed.  Per
 * counted day (t >= flow.pop.t_first), days ascending, one chain each per (c, b), no atomics, every product written here
 * rounded once:
 *   r = v - o2      d = v - m2      e = o2 - m2           o2 = aux_target[t,b], m2 = aux_shift[b]
 *   sse = fmaf(w * r, r, sse)                             -> aux_sse
 *   s1  = fmaf(w,     d, s1)                              -> aux_s1
 *   s2  = fmaf(w * d, d, s2)                              -> aux_s2
 *   s3  = fmaf(w * d, e, s3)                              -> aux_s3      (w = aux_w[t,b], 1 when aux_w is NULL)
 * aux_shift is meant to be the weighted mean of aux_target, as `shift` is of the flow target; masking is the caller's
 * job here too (w = 0 does not neutralise a NaN in aux_target).  csrc/hbv_pop.h has the kernel and the arithmetic
 * (hbvx_popk::AuxStats).
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) a candidate's eight numbers and both series do not
 * depend on n_cand or on the other candidates; (3) flow.pop.sim == NULL or aux_sim == NULL changes no bit of anything
 * else; (4) flow.pop.cost, flow.s1..s3 and flow.pop.sim have the bits hbvx_population_stats gives for the same candidate
 * and transform; (5) argument errors are reported before anything is launched: hbvx_population_stats', and HBVX_E_NULL
 * (pj, aux_target, aux_shift, aux_sse, aux_s1, aux_s2, aux_s3), HBVX_E_UNSUPPORTED (an aux_series other than
 * HBVX_F_Q0, _Q1, _Q2, _AET, _SWE: HBVX_F_QSIM is the flow term, HBVX_F_RECHARGE .. HBVX_F_CAPILLARY are not offered).
 * Not built: HBVX_MODEL_HBVADJ (its population kernel is a separate family: hbvx_adj_population_period scores one of
 * its storages) and HBVX_MODEL_HOURLY (HBVX_E_UNSUPPORTED),
 * a transform of the aux value, more than one aux series per launch, sums over several days before the comparison. */
typedef struct hbvx_pop_joint {
    hbvx_pop_stats flow;           /* the flow term: hbvx_population_stats' argument, unchanged in meaning */
    int32_t aux_series;            /* HBVX_F_Q0, HBVX_F_Q1, HBVX_F_Q2, HBVX_F_AET or HBVX_F_SWE */
    const float *aux_target;       /* [T - t_first, B], required */
    const float *aux_w;            /* [T - t_first, B] or NULL (= 1) */
    const float *aux_shift;        /* [B], required */
    float *aux_sse, *aux_s1, *aux_s2, *aux_s3;     /* [P,B] each, overwritten completely */
    float *aux_sim;                /* optional [P, T - t_first, B]: each candidate's aux series */
} hbvx_pop_joint;                  /* hbvx_sizeof(12) */
int hbvx_population_joint(const hbvx_desc *d, const hbvx_pop_joint *pj, void *stream);

/* Population scores against period means (optional export; a library may lack it): hbvx_population_joint with each of
 * the two series averaged over the periods of a calendar of its own -- 8-day composites, months -- before it meets its
 * target.  The model, the candidates, the ensemble means y (routed flow) and v (aux flux), the routing and t_first are
 * hbvx_population_joint's; the routing runs on every day.  A calendar is an ascending array of closing days relative to
 * t_first: period k covers the scored days after end[k-1] (period 0: from day 0) up to and including end[k]; days after
 * the last closing day are simulated and scored nowhere.  Per series, days ascending, with n the period's day count:
 *   acc = x                      (the period's first day: assigned)           x = y | v
 *   acc = acc + x                (its later days)
 *   mean = acc / (float)n        (the day that closes period k: one division; a one-day period gives x bit for bit)
 * and on that day one step of the four chains, periods ascending, every product written here rounded once:
 *   flow:  y' = mean | sqrtf(mean) | logf(mean + eps[b])     (the transform of the period MEAN)
 *          r = y' - o'      d = y' - m      e = o' - m       o' = flow.pop.target[k,b], m = flow.shift[b]
 *          sse = fmaf(w * r, r, sse)   s1 = fmaf(w, d, s1)   s2 = fmaf(w * d, d, s2)   s3 = fmaf(w * d, e, s3)
 *                                                            (w = flow.pop.w[k,b], 1 when NULL)
 *   aux:   the same four lines on mean itself against aux_target[k,b], aux_shift[b], aux_w[k,b]: never transformed.
 * Targets, weights and the optional series are indexed by PERIOD: flow.pop.target / w [KF,B], flow.pop.sim [P,KF,B],
 * aux_target / aux_w [KA,B], aux_sim [P,KA,B]; the series hold the period means (the flow's before its transform).
 * Rows of a series whose period never closes are not written.  joint.aux_series == HBVX_POP_NO_AUX: there is no aux
 * term; the aux pointers, n_aux_periods and aux_end are then not read and nothing aux is written, and the flow numbers
 * have the bits they have with an aux term.
 * Guarantees: those of hbvx_population_joint (1)-(3), for all eight outputs and both series; (4) with both calendars
 * daily (end[k] = k, K = T - t_first) every output has hbvx_population_joint's bits; (5) the kernel is memory-safe for
 * any calendar content: no closing day and no target row beyond its count is read, and a calendar that does not ascend
 * only leaves periods unclosed; (6) argument errors are reported before anything is launched: hbvx_population_joint's
 * (its aux rules only when there is an aux term), and HBVX_E_NULL (pq, flow_end; aux_end with an aux term),
 * HBVX_E_SHAPE (n_flow_periods, or n_aux_periods with an aux term, outside 1..T - t_first), HBVX_E_UNSUPPORTED (an
 * aux_series that is neither HBVX_POP_NO_AUX nor one of the five).  csrc/hbv_pop.h has the kernel and
 * the arithmetic (hbvx_popk::PeriodMean, BasinStats::score, AuxStats::push).
 * Not built: period sums as an input form (divide by the lengths), per-basin calendars, HBVX_MODEL_HOURLY;
 * HBVX_MODEL_HBVADJ has hbvx_adj_population_period below. */
#define HBVX_POP_NO_AUX (-1)

typedef struct hbvx_pop_period {
    hbvx_pop_joint joint;          /* both terms as above, targets / weights / series per period */
    int32_t n_flow_periods;        /* KF, 1..T - t_first */
    const int32_t *flow_end;       /* [KF] device array: closing days relative to t_first, ascending */
    int32_t n_aux_periods;         /* KA, 1..T - t_first; not read without an aux term */
    const int32_t *aux_end;        /* [KA] device array; not read without an aux term */
} hbvx_pop_period;                 /* hbvx_sizeof(13) */
int hbvx_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream);

/* Population evaluation of the implicit scheme (optional exports; a library may lack them): hbvx_population_cost and
 * hbvx_population_stats for HBVX_MODEL_HBVADJ, on the same structs.  For every candidate c and basin b the day loop of
 * hbvx_adj_forward's one-wave kernel runs on `d` -- per lane and day the system G(x) = 0 is solved in registers by the
 * day function d->adj_stop selects (2: the staged solve; 0: the joint Newton iteration with the per-lane stopping
 * rule), under d->adj_gtol / d->adj_max_iter -- with the candidate's static values in place of d->p[i].sta wherever
 * pop->p[i].sta is set.  Dynamic parameters, the drop masks (per LANE in this model: drop[b*M + j]), state_in (NULL:
 * zeros) and the forcings are the descriptor's, shared by all candidates.  Per day
 *   Q = (q0 + q1) + q2 at the solved state,   q = sum over the members of Q (xor butterfly) * (1 / M),
 * and from there on everything is hbvx_population_cost's / hbvx_population_stats' text above: the gamma unit hydrograph
 * of (c, b), the causal 15-day window, t_first, the residual chain cost = fmaf(w * r, r, cost), the transform and the
 * three moment chains, `sim`.  csrc/hbv_adj_pop.h has the kernel.
 * Guarantees: (1) two calls on the same inputs give the same bits; (2) the bits of cost[c,b], s1..s3[c,b] and
 * sim[c,:,b] do not depend on n_cand or on the other candidates; (3) sim == NULL changes no bit; (4) under
 * HBVX_POP_T_NONE pop.cost of hbvx_adj_population_stats has the bits hbvx_adj_population_cost gives, and `sim` has
 * them under every transform; (5) argument errors are reported before anything is launched.
 * Errors: those of hbvx_population_cost / hbvx_population_stats, except that the model must be HBVX_MODEL_HBVADJ
 * (else HBVX_E_UNSUPPORTED), and: HBVX_E_SHAPE (adj_gtol < 0 or NaN, adj_max_iter outside 0..64, adj_stop outside
 * 0..2), HBVX_E_UNSUPPORTED (adj_stop == 1: the batch-wide stopping rule votes over the 64 lanes of a wave, and a
 * candidate's cost must not depend on which basins share its wave; a non-NULL d->muwts: the implicit scheme has no
 * ensemble weights).
 * Bit equality with hbvx_adj_forward + hbvx_route_forward is not promised: the forward may be taken by another kernel
 * family (the tiled stepper, the staged pipeline). */
int hbvx_adj_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream);
int hbvx_adj_population_stats(const hbvx_desc *d, const hbvx_pop_stats *ps, void *stream);

/* Population scores of the implicit scheme against period means, with an optional observed STORAGE beside streamflow
 * (optional export; a library may lack it): hbvx_population_period for HBVX_MODEL_HBVADJ, on the same struct.  The day
 * loop, the candidates, the Newton policy, Q and its ensemble mean q are hbvx_adj_population_stats'; the routing runs on
 * every day; the calendars, the period means, the transform of the flow's period mean, the eight chains, the per-PERIOD
 * targets / weights / series and HBVX_POP_NO_AUX are hbvx_population_period's, line by line.  What differs is the aux
 * value: the implicit scheme solves for its five storages every day, and the aux value of a day is the ensemble mean
 * of one of them at the day's solved state,
 *   v = (sum over the members of x[k]) * (1 / M),   k = joint.aux_series = HBVX_ADJ_AUX_SNOWPACK .. HBVX_ADJ_AUX_SLZ,
 * the RAW x[k] -- what hbvx_adj_forward writes to row t + 1 of its trajectory, not the value clamped at zero that
 * enters Q -- never routed and never transformed.  Fluxes (evapotranspiration, the runoff components) are not offered:
 * the staged solve does not keep them.
 * Guarantees: hbvx_population_period's (1)-(3) and (5); (4) with both calendars daily and no aux term, pop.cost,
 * s1..s3 and pop.sim have hbvx_adj_population_stats' bits; with an aux term the flow outputs keep theirs; (6) argument
 * errors are reported before anything is launched: hbvx_adj_population_stats' (the model, the Newton policy,
 * adj_stop == 1, muwts) and hbvx_population_period's, with HBVX_E_UNSUPPORTED for an aux_series that is neither
 * HBVX_POP_NO_AUX nor a storage index 0..4.  csrc/hbv_adj_pop.h has the kernel.
 * Not built: fluxes as the aux series, a transform of the aux value, more than one aux series per launch, period sums,
 * per-basin calendars. */
#define HBVX_ADJ_AUX_SNOWPACK 0
#define HBVX_ADJ_AUX_MELTWATER 1
#define HBVX_ADJ_AUX_SM 2
#define HBVX_ADJ_AUX_SUZ 3
#define HBVX_ADJ_AUX_SLZ 4
int hbvx_adj_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream);

/* Zero `bytes` bytes at `ptr` (streaming non-temporal stores).  The autograd contract of the plug-in wants
 * gradient tensors shaped like the raw parameter tensor [T,B,ny] (hbv.py:211-246: static parameters read
 * one row of it), so the dense zero fill is part of every backward step. */
int hbvx_zero(void *ptr, uint64_t bytes, void *stream);

/* The same for a gradient buffer of which hbvx_backward will overwrite a part: `ptr` is a dense
 * [rows, width] float matrix (rows = T*B of the raw parameter tensor, width = ny); every element is zeroed
 * EXCEPT those with r0 <= row < r1 and column in a kept group -- column c belongs to group c / group_w,
 * group g (< 32) is kept when bit g of `keep_groups` is set.  Those are exactly the elements the
 * adjoint stores (never accumulates) for a dynamic parameter: rows = the days of the call, group =
 * the parameter's nmul columns (hbv.py:201-208).  With every parameter dynamic (BASELINE config 3)
 * this removes a 4.4 GB fill per step.  keep_groups == 0 is hbvx_zero. */
int hbvx_zero_except(float *ptr, int64_t rows, int32_t width, int64_t r0, int64_t r1, int32_t group_w,
                     uint32_t keep_groups, void *stream);

/* Diagnostics (tests only): out[i] = the device pow used for (SM/FC)**BETA on x[i], y[i]. */
int hbvx_selftest_pow(const float *x, const float *y, float *out, int n, void *stream);
/* Diagnostics (tests only): out[i] = the device quotient used for SM/FC on x[i] / y[i]. */
int hbvx_selftest_div(const float *x, const float *y, float *out, int n, void *stream);
/* Diagnostics (tests only): out[i] = y' as hbvx_population_stats forms it from y[i] (and eps[i] under HBVX_POP_T_LOG;
 * eps may be NULL otherwise). */
int hbvx_selftest_pop_transform(const float *y, const float *eps, float *out, int n, int transform, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HBVX_H */
