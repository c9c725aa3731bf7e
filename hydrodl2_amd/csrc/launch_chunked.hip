// launch_chunked.hip -- host dispatch of the time-parallel adjoint (hbv_chunked.h).
#include "hbvx_host.h"
#include "hbv_chunked.h"

#include <algorithm>
#include <atomic>

using namespace hbvx;
using namespace hbvx_host;

namespace hbvx_host {
void launch_chunk_scan(const hbvx::ChunkArgs &a, hipStream_t st)
{
    const int64_t N = (int64_t)a.d.B * a.d.M;
    hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, a);
}
void launch_chunk_reduce(const hbvx::ChunkArgs &a, int n_param, hipStream_t st)
{
    const int64_t N = (int64_t)a.d.B * a.d.M;
    hipLaunchKernelGGL(k_bwd_chunk_reduce, dim3((unsigned)((N + 255) / 256), n_param), dim3(256), 0, st, a, n_param);
}
}

int hbvx_host::chunk_days() { int c = env_int("HBVX_CHUNK", 64); return c < 2 ? 2 : c; }

bool hbvx_host::chunked_applicable(const hbvx_desc *d)
{
    const char *v = getenv("HBVX_BWD");
    if (v && !strcmp(v, "tiled")) return false;
    return d->T >= 2 * chunk_days();
}

static int np_of(const hbvx_desc *d) { return d->n_param; }

// Whether the descriptor admits the one-pass static adjoint (hbv_chunked.h, k_bwd_chunk_onepass): HBV 1.0 with every
// parameter static.  (The call must also have no learned ensemble weights and no forcing gradient; the workspace is
// sized on the descriptor's model and parameters alone, so that its size does not depend on those or on the knob.)
static bool onepass_admitted(const hbvx_desc *d)
{
    return d->model == HBVX_MODEL_HBV10 && (d->n_param == 12 || d->n_param == 13) && count_dyn(d) == 0;
}

// per-chunk rows of static-gradient partials: the two-pass sweep's NP, or the one-pass form's G_c and g0_c
static int gpart_rows(const hbvx_desc *d)
{
    const int np = np_of(d);
    return onepass_admitted(d) ? std::max(np, onepass_rows(np)) : np;
}

extern "C" uint64_t hbvx_backward_workspace_bytes(const hbvx_desc *d)
{
    if (!d || d->T <= 0 || d->B <= 0 || d->M <= 0 || !chunked_applicable(d)) return 0;
    const int C = chunk_days();
    const uint64_t nchunk = (uint64_t)(d->T + C - 1) / C;
    return nchunk * (uint64_t)d->B * (uint64_t)d->M * (uint64_t)(35 + gpart_rows(d)) * sizeof(float);
}

// Which form of the time-parallel adjoint the last chunked call ran: 1 one-pass, 2 two-pass (0: none yet).
// hbvx_last_dispatch(1) says "chunked" for both.
static std::atomic<int> g_chunk_form{0};
extern "C" int hbvx_chunk_form(void) { return g_chunk_form.load(); }

// Chunks composed per workgroup of the one-pass form (hbv_chunked.h, k_bwd_chunk_onepass).  HBVX_ONEPASS_GROUP is a
// test / tool knob like HBVX_CHUNK_ONEPASS; 1 writes one map per chunk.  Default: profiles/r15_onepass_group.md.
#define ONEPASS_GROUP_DEFAULT 4
static int onepass_group() { return std::min(std::max(env_int("HBVX_ONEPASS_GROUP", ONEPASS_GROUP_DEFAULT), 1), ONEPASS_GMAX); }
// Diagnostics for tests and tools: the group size of the last one-pass call (0: none yet), and the LDS a workgroup of
// a grouped call takes (its hand-over slot) for a model of n_param parameters.
static std::atomic<int> g_onepass_group{0};
extern "C" int hbvx_onepass_group(void) { return g_onepass_group.load(); }
extern "C" int hbvx_onepass_slot_bytes(int n_param) { return onepass_slot_bytes(n_param); }
// ... and the rows of grad_flux4 its day loop loaded: 4, or what hbvx_backward_live said (k_bwd_chunk_onepass_live)
static std::atomic<int> g_onepass_live{0};
extern "C" int hbvx_onepass_live_rows(void) { return g_onepass_live.load(); }

template <int MODEL, bool BETAET, int DYN, bool GFULL>
static hipError_t launch_chunked_t(const ChunkArgs &a, hipStream_t st, bool onepass, int n_live)
{
    const hbvx_desc &d = a.d;
    const int bpw = 64 >> a.lgMp;
    const int64_t N = (int64_t)d.B * d.M;
    (void)bpw;
    dim3 g2((unsigned)(8 * a.per_xcd * a.nchunk));      // XCD-aware 1-D block map (hbv_chunked.h::chunk_block)
    if constexpr (MODEL == MODEL_HBV10 && DYN == 0) {
        if (onepass) {   // static parameters only: the trajectory is read once (hbv_chunked.h, k_bwd_chunk_onepass)
            constexpr int NP = ChunkNP<MODEL, BETAET>::value;
            g_chunk_form = 1;
            ChunkArgs o = a;            // a workgroup per group of o.group chunks, composed into one map on chip
            o.group = onepass_group();
            g_onepass_group = o.group;
            const int ngrp = (a.nchunk + o.group - 1) / o.group;
            const dim3 og((unsigned)(8 * a.per_xcd * ngrp)), ob(64 * o.group);
            const int olds = o.group > 1 ? onepass_slot_bytes(NP) : 0;
            // hbvx_backward_live: the instance that loads only the rows of grad_flux4 that exist (runoff-only loss)
            const int live = GFULL ? 4 : n_live;
            g_onepass_live = live;
            if constexpr (!GFULL) {
                if (live == 1) hipLaunchKernelGGL((k_bwd_chunk_onepass_live<BETAET, 1>), og, ob, olds, st, o);
                if (live == 2) hipLaunchKernelGGL((k_bwd_chunk_onepass_live<BETAET, 2>), og, ob, olds, st, o);
                if (live == 3) hipLaunchKernelGGL((k_bwd_chunk_onepass_live<BETAET, 3>), og, ob, olds, st, o);
            }
            if (live >= 4) hipLaunchKernelGGL((k_bwd_chunk_onepass<BETAET, GFULL>), og, ob, olds, st, o);
            ChunkArgs s = a;            // scan and fold walk the groups' maps and boundary adjoints
            s.nchunk = ngrp;
            hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, s);
            store_gate(&a.io, st);
            const int ngroup = (ngrp + ONEPASS_FOLD_GROUP - 1) / ONEPASS_FOLD_GROUP;
            hipLaunchKernelGGL((k_bwd_chunk_fold<NP>), dim3((unsigned)((N + 255) / 256), (unsigned)ngroup), dim3(256), 0,
                               st, s);
            ChunkArgs r = a;            // the fold's partials, in the maps' rows (hbv_chunked.h, B4 of the one-pass form)
            r.gpart = a.phi;
            r.nchunk = ngroup;
            hipLaunchKernelGGL(k_bwd_chunk_reduce, dim3((unsigned)((N + 255) / 256), d.n_param), dim3(256), 0, st,
                               r, d.n_param);
            return hipGetLastError();
        }
    }
    g_chunk_form = 2;
    // the two slot lists users actually run get compile-time slots (hbv_chunked.h::SlotCombo)
    int sc = 0;
    const bool mu = d.muwts != nullptr;     // (the compiled slot combos have no MU instance: the slot-list form below)
    if (!mu && DYN == 1 && MODEL == MODEL_HBV10 && BETAET && a.nd == 2 && a.dslot[0] == P_BETA && a.dslot[1] == P_BETAET) sc = 1;
    if (!mu && DYN == 1 && (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) && a.nd == 3 && a.dslot[0] == P_BETA &&
        a.dslot[1] == P_K0 && a.dslot[2] == P_BETAET)
        sc = 2;
    if constexpr (DYN == 1 && MODEL == MODEL_HBV10 && BETAET) {
        if (sc == 1) {
            hipLaunchKernelGGL((k_bwd_chunk_phi<MODEL, BETAET, DYN, GFULL, 1>), g2, dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, a);
            store_gate(&a.io, st);
            hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL, 1>), g2, dim3(64), 0, st, a);
        }
    }
    if constexpr (DYN == 1 && (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY)) {
        if (sc == 2) {
            hipLaunchKernelGGL((k_bwd_chunk_phi<MODEL, BETAET, DYN, GFULL, 2>), g2, dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, a);
            store_gate(&a.io, st);
            hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL, 2>), g2, dim3(64), 0, st, a);
        }
    }
    if (sc != 0) {
        hipLaunchKernelGGL(k_bwd_chunk_reduce, dim3((unsigned)((N + 255) / 256), d.n_param), dim3(256), 0, st,
                           a, d.n_param);
        return hipGetLastError();
    }
    if constexpr (DYN == 0 || DYN == 1) {
        if (d.muwts) {    // learned ensemble weights: the MU instances of the static / slot-list modes (hbv_chunked.h)
            hipLaunchKernelGGL((k_bwd_chunk_phi<MODEL, BETAET, DYN, GFULL, 0, true>), g2, dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, a);
            store_gate(&a.io, st);
            hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL, 0, false, true>), g2, dim3(64), 0, st, a);
            hipLaunchKernelGGL(k_bwd_chunk_reduce, dim3((unsigned)((N + 255) / 256), d.n_param), dim3(256), 0, st,
                               a, d.n_param);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_bwd_chunk_phi<MODEL, BETAET, DYN, GFULL>), g2, dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_bwd_chunk_scan, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, a);
    store_gate(&a.io, st);       // phi and scan only read; the sweep stores
    if constexpr (DYN == 3) {
        // whole-row gradient stores when every parameter's gradient sits in one [T,B,ny] tensor in the
        // reference's column order, rows 8-byte aligned (hbv_chunked.h, ROWST)
        const hbvx_param_grad &g0 = a.io.g[0];
        bool rows = g0.dyn && ((uintptr_t)g0.dyn & 7) == 0 &&
                    (g0.dyn_b_stride & 1) == 0 && (g0.dyn_t_stride & 1) == 0 && ((d.n_param * d.M) & 1) == 0;
        for (int i = 1; i < d.n_param && rows; i++)
            rows = a.io.g[i].dyn == g0.dyn + (int64_t)i * d.M && a.io.g[i].dyn_b_stride == g0.dyn_b_stride &&
                   a.io.g[i].dyn_t_stride == g0.dyn_t_stride;
        if (rows) hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL, 0, true>), g2, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL>), g2, dim3(64), 0, st, a);
        return hipGetLastError();   // every parameter dynamic: the static gradient is zero
    }
    hipLaunchKernelGGL((k_bwd_chunk_sweep<MODEL, BETAET, DYN, GFULL>), g2, dim3(64), 0, st, a);
    if (DYN == 3) return hipGetLastError();   // every parameter dynamic: the static gradient is zero
    hipLaunchKernelGGL(k_bwd_chunk_reduce, dim3((unsigned)((N + 255) / 256), d.n_param), dim3(256), 0, st,
                       a, d.n_param);
    return hipGetLastError();
}

template <int DYN, bool GFULL>
static hipError_t launch_chunked_v(const hbvx_desc *d, const ChunkArgs &a, hipStream_t st, bool onepass = false,
                                   int n_live = 4)
{
    return with_model(d, [&](auto m, auto be) { return launch_chunked_t<m, be, DYN, GFULL>(a, st, onepass, n_live); });
}

// Whether this call runs the one-pass form (HBVX_CHUNK_ONEPASS=0, a test / tool knob: the two-pass form instead)
static bool onepass_takes(const hbvx_desc *d, const hbvx_bwd_io *io)
{
    return onepass_admitted(d) && !d->muwts && !io->grad_x && env_int("HBVX_CHUNK_ONEPASS", 1) != 0;
}

static hipError_t launch_chunked(const hbvx_desc *d, const hbvx_bwd_io *io, hipStream_t st, int n_live)
{
    ChunkArgs a;
    a.d = *d;
    a.io = *io;
    a.lgMp = lg_members(d->M);
    a.C = chunk_days();
    a.nchunk = (d->T + a.C - 1) / a.C;
    a.per_xcd = chunk_per_xcd(d->B, a.lgMp);
    a.group = 1;
    const int64_t N = (int64_t)d->B * d->M;
    a.phi = (float *)io->workspace;
    a.abnd = a.phi + (int64_t)a.nchunk * 30 * N;
    a.gpart = a.abnd + (int64_t)a.nchunk * 5 * N;
    const bool gfull = io->grad_flux != nullptr;
    a.nd = 0;
    a.dslot[0] = a.dslot[1] = a.dslot[2] = 0;
    const int ndyn = count_dyn(d);
    if (ndyn > 0 && ndyn <= CHUNK_FEW) {   // few dynamic parameters: slot-list kernels (muwts: a run-time flag in them)
        for (int i = 0; i < d->n_param; i++)
            if (d->p[i].dyn) a.dslot[a.nd++] = i;
        return gfull ? launch_chunked_v<1, true>(d, a, st) : launch_chunked_v<1, false>(d, a, st);
    }
    // "all" mode: every parameter dynamic, no dy_drop mask, no muwts, and all rows in ONE tensor with the reference's
    // column order (hbv_chunked.h::chunk_dma_dyn addresses them from parameter 0's pointer and strides)
    bool alldyn = ndyn == d->n_param && !d->muwts;
    for (int i = 0; i < d->n_param && alldyn; i++)
        alldyn = d->p[i].drop == nullptr && d->p[i].dyn == d->p[0].dyn + (int64_t)i * d->M &&
                 d->p[i].dyn_t_stride == d->p[0].dyn_t_stride && d->p[i].dyn_b_stride == d->p[0].dyn_b_stride;
    if (alldyn) return gfull ? launch_chunked_v<3, true>(d, a, st) : launch_chunked_v<3, false>(d, a, st);
    if (ndyn > 0) return gfull ? launch_chunked_v<2, true>(d, a, st) : launch_chunked_v<2, false>(d, a, st);
    const bool onepass = onepass_takes(d, io);
    return gfull ? launch_chunked_v<0, true>(d, a, st, onepass) : launch_chunked_v<0, false>(d, a, st, onepass, n_live);
}

bool hbvx_host::try_bwd_chunked(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc, int n_live)
{
    if (io->workspace && chunked_applicable(d) && io->workspace_bytes >= hbvx_backward_workspace_bytes(d)) {
        // hbvx_backward_live: fewer than four rows of grad_flux4 -- only the one-pass form with the runoff-only loss
        // knows (hbv_chunked.h, LIVE); every other kernel of this family reads four rows
        if (n_live < 4 && !(onepass_takes(d, io) && !io->grad_flux)) {
            *rc = fail(HBVX_E_UNSUPPORTED, "live rows: the one-pass static adjoint does not take this call");
            return true;
        }
        hipError_t e = launch_chunked(d, io, (hipStream_t)stream, n_live);
        note_dispatch(1, "chunked");
        *rc = e != hipSuccess ? hip_fail(e, "hbvx_backward (chunked) launch") : HBVX_OK;
        return true;
    }
    return false;
}
