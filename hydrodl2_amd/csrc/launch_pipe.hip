// launch_pipe.hip -- host dispatch of the pipelined forward (hbv_pipe.h).
#include "hbvx_host.h"
#include "hbv_pipe.h"

using namespace hbvx;
using namespace hbvx_host;

// Static parameters, PIPE_KT_STATIC days per tile: the three-stage tile (HBV 1.0; the implicit scheme has ten days) takes 157 696 B,
// the two-stage one with the capillary row 163 328 B -- exactly LDS_BUDGET, 512 B under the CU's 160 KB.  A row or a
// day more and the launcher below would hand those models to the tiled forward without a word: fail the build instead.
static_assert(PipeLds(PIPE_KT_STATIC).total * 4 <= LDS_BUDGET && PipeLds(PIPE_KT_STATIC, 0, true).total * 4 <= LDS_BUDGET,
              "static pipelined tiles must fit LDS_BUDGET with and without the capillary row");

bool hbvx_host::try_fwd_pipe(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream, int *rc)
{
        // HBV 1.0 / 1.1p / 2.0, at most PIPE_MAXDYN dynamic parameters, flux requested: pipelined
        // forward (hbv_pipe.h; three stages for HBV 1.0, two for the capillary models)
        const char *fv = getenv("HBVX_FWD");
        const bool adj = d->model == HBVX_MODEL_HBVADJ;   // implicit scheme, staged solve (hbvx_adj_forward only)
        // staged rows per day: the dynamic parameters' and, behind them, the learned ensemble weights `muwts`
        // (hbv_pipe.h: has_mu); "nd" below counts both
        const bool mu = d->muwts != nullptr && !adj;
        const int nd = count_dyn(d) + (mu ? 1 : 0);
        const bool many = nd > PIPE_FEWDYN;          // 4-day tiles, several staged rows per filler wave
        const int Kt = many ? PIPE_KT_MANY : (nd > 0 ? PIPE_KT : (adj ? PIPE_KT_STATIC_ADJ : PIPE_KT_STATIC));
        const bool cap = d->model != HBVX_MODEL_HBV10 && !adj;
        const int nfl = adj ? 1 : (cap ? 12 : 11);
        // per-lane and per-tile byte offsets are 32-bit in the pipelined kernel
        bool off32 = ((int64_t)d->B * d->x_b_stride + (int64_t)Kt * d->x_t_stride) * 4 < (int64_t)1 << 31;
        for (int i = 0; i < d->n_param; i++)
            if (d->p[i].dyn)
                off32 = off32 && ((int64_t)d->B * d->p[i].dyn_b_stride + (int64_t)Kt * d->p[i].dyn_t_stride) * 4 <
                                     (int64_t)1 << 31;
        if (mu) off32 = off32 && ((int64_t)d->B * d->mu_b_stride + (int64_t)Kt * d->mu_t_stride) * 4 < (int64_t)1 << 31 &&
                        d->mu_t_stride >= 0;
        // the kernel's buffer descriptors span `rows` day strides from a tile's first day (hbv_pipe.h, rsrc_of), and a
        // load outside that range returns 0: every basin's values must lie within its day's stride -- the day the
        // outer dimension of x and of each staged row.  A [B,T,3] buffer viewed as [T,B,3] is not: the tiled forward
        const int chmax = std::max(d->ch_prcp, std::max(d->ch_tmean, d->ch_pet));
        bool day_outer = (int64_t)(d->B - 1) * d->x_b_stride + chmax + 1 <= d->x_t_stride;
        for (int i = 0; i < d->n_param; i++)
            if (d->p[i].dyn)
                day_outer = day_outer && (int64_t)(d->B - 1) * d->p[i].dyn_b_stride + d->M <= d->p[i].dyn_t_stride;
        if (mu) day_outer = day_outer && (int64_t)(d->B - 1) * d->mu_b_stride + d->M <= d->mu_t_stride;
        const int64_t wgs_p = ((int64_t)d->B + (64 >> lg_members(d->M)) - 1) / (64 >> lg_members(d->M));
        const bool pmodel = d->model == HBVX_MODEL_HBV10 || d->model == HBVX_MODEL_HBV11P ||
                            d->model == HBVX_MODEL_HBV20 || d->model == HBVX_MODEL_HOURLY ||
                            (adj && d->adj_stop == 2 && !many);
        const size_t lds = (size_t)PipeLds(Kt, nd > 0 ? (many ? nd : PIPE_FEWDYN) : 0, cap).total * 4;
        // HBVX_TRAJ_CKPT: the row drainers keep every K-th day only
        const int ckpt_k = (out->traj && HBVX_TRAJ_KIND(out->traj_layout) == HBVX_TRAJ_CKPT)
                               ? HBVX_TRAJ_CKPT_DAYS(out->traj_layout) : 0;
        const bool ckpt_fits = !ckpt_k || ((int64_t)((d->T + ckpt_k - 1) / ckpt_k) * 5 * d->B * d->M * 4 < (int64_t)1 << 32);
        if (ckpt_fits && use_tiled(d) && !(fv && !strcmp(fv, "tiled")) && pmodel && off32 && day_outer &&
            nd <= PIPE_MAXDYN && (int)lds <= LDS_BUDGET && wgs_p < 4096 && !(adj && d->muwts) && (out->flux || adj) && d->T >= 4 * Kt &&
            !(adj && ckpt_k) &&
            (int64_t)d->B * d->M * 4 * Kt < (int64_t)1 << 31 &&
            (int64_t)nfl * d->T * d->B * 4 < (int64_t)1 << 31) {
            PipeArgs pa;
            pa.d = *d;
            pa.o = *out;
            pa.lgMp = lg_members(d->M);
            pa.Kt = Kt;
            pa.ckptK = ckpt_k;
            const int bpw_p = 64 >> pa.lgMp;
            dim3 grid_p((d->B + bpw_p - 1) / bpw_p);
            // hbvx_fwd_out.zero_ptr: surplus workgroups of THIS launch write its zeros while the recurrence runs -- when the
            // chain leaves at least an eighth of the chip idle (config 2: 168 workgroups, one per CU, 88 CUs free).
            // HBVX_PIPE_FILL_WGS: 0 = never (everything is left to hbvx_zero_rest), n = that many fill workgroups;
            // HBVX_PIPE_FILL_WAVES: waves of each that write (tools: the fill's share of HBM)
            pa.fill_ptr = nullptr;
            pa.fill_state = nullptr;
            pa.fill_n16 = 0;
            pa.nwg = (int)grid_p.x;
            pa.fill_waves = env_int("HBVX_PIPE_FILL_WAVES", 16);
            if (out->zero_ptr && out->zero_state && out->zero_bytes >= 16 && ((uintptr_t)out->zero_ptr & 15) == 0) {
                const int n_cu = device_cu_count();
                const int spare = n_cu - (int)grid_p.x;
                const int nfill = env_int("HBVX_PIPE_FILL_WGS", spare >= n_cu / 8 ? spare : 0);
                if (nfill > 0) {
                    pa.fill_ptr = out->zero_ptr;
                    pa.fill_state = (unsigned *)out->zero_state;
                    pa.fill_n16 = out->zero_bytes / 16;     // a ragged tail (< 16 bytes) belongs to hbvx_zero_rest
                    grid_p.x += (unsigned)nfill;
                    zero_taken() = true;
                }
            }
            int pthreads = env_int("HBVX_PIPE_THREADS", 1024); // 3 steppers + filler + drainers (hbv_pipe.h)
            pthreads = pthreads < 512 ? 512 : (pthreads > 1024 ? 1024 : (pthreads / 64) * 64);
            if (nd > 0) pthreads = 1024;   // the dynamic-parameter roles assume all 16 waves
            const bool be = d->n_param == 13, tr = out->traj != nullptr, dy = nd > 0;
            // who stores the trajectory (hbv_pipe.h, TRAJ): the steppers themselves where the reducers are the busy
            // helpers -- 8 or more basins per wave (ensembles of at most 8 members); HBVX_PIPE_DIRECT=0|1 pins it (tools)
            const int dflag = env_int("HBVX_PIPE_DIRECT", -1);
            const bool direct = dflag >= 0 ? dflag != 0 : bpw_p >= 8;
            hipStream_t st = (hipStream_t)stream;
            // compile-time dynamic sets (hbv_pipe.h, SC): {BETA, BETAET} and {BETA, K0, BETAET}
            unsigned dmask = 0;
            for (int i = 0; i < d->n_param; i++) dmask |= d->p[i].dyn ? (1u << i) : 0u;
            const int sc = dmask == ((1u << P_BETA) | (1u << P_BETAET)) ? 1
                         : dmask == ((1u << P_BETA) | (1u << P_K0) | (1u << P_BETAET)) ? 2 : 0;
            // the instance for one (model, BETAET, trajectory mode), all three as std::integral_constant
            auto go = [&](auto m, auto be_c, auto trm) -> hipError_t {
                constexpr int MODEL = decltype(m)::value, TR = decltype(trm)::value;
                constexpr bool BE = decltype(be_c)::value;
                // the compiled sets: {BETA, BETAET} for HBV 1.0 with BETAET and 1.1p, {BETA, K0, BETAET} for HBV 1.0
                // with BETAET, 2.0 and hourly
                constexpr bool S1 = BE && (MODEL == MODEL_HBV10 || MODEL == MODEL_HBV11P);
                constexpr bool S2 = BE && (MODEL == MODEL_HBV10 || MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY);
                auto launch = [&](auto kern) { return launch_tiled_one(kern, pa, grid_p, pthreads, lds, st); };
                if constexpr (MODEL != MODEL_HBVADJ)    // (HBVADJ: at most PIPE_FEWDYN dynamic parameters, pmodel)
                    if (many) return launch(k_fwd_pipe<MODEL, BE, TR, true, true, 0>);
                if constexpr (S1)
                    if (dy && sc == 1) return launch(k_fwd_pipe<MODEL, BE, TR, true, false, 1>);
                if constexpr (S2)
                    if (dy && sc == 2) return launch(k_fwd_pipe<MODEL, BE, TR, true, false, 2>);
                if (dy) return launch(k_fwd_pipe<MODEL, BE, TR, true, false, 0>);
                return launch(k_fwd_pipe<MODEL, BE, TR, false, false, 0>);
            };
            constexpr std::integral_constant<int, 0> tr0{};
            constexpr std::integral_constant<int, 1> tr1{};
            constexpr std::integral_constant<int, 2> tr2{};
            hipError_t e;
            if (adj) {   // HBVADJ's own instances (descriptor flags): the drained row trajectory or none
                constexpr std::integral_constant<int, MODEL_HBVADJ> ma{};
                if (be) e = tr ? go(ma, std::true_type{}, tr1) : go(ma, std::true_type{}, tr0);
                else e = tr ? go(ma, std::false_type{}, tr1) : go(ma, std::false_type{}, tr0);
            } else {
                e = with_model(d, [&](auto m, auto be_c) {
                    return tr && direct ? go(m, be_c, tr2) : (tr ? go(m, be_c, tr1) : go(m, be_c, tr0));
                });
            }
            note_dispatch(0, "pipe");
            *rc = e != hipSuccess ? hip_fail(e, "hbvx_forward (pipelined) launch") : HBVX_OK;
            return true;
        }
    return false;
}

#ifdef PIPE_PROBE
extern "C" int hbvx_debug_pipe_blocks(unsigned long long *out, int n)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(hbvx::g_pipe_blocks), (size_t)(n > 4096 ? 4096 : n) * sizeof(unsigned long long));
    return e == hipSuccess ? 0 : -1;
}
extern "C" int hbvx_debug_pipe_probe(unsigned long long *out32)
{
    hipError_t e = hipMemcpyFromSymbol(out32, HIP_SYMBOL(hbvx::g_pipe_probe), 32 * sizeof(unsigned long long));
    return e == hipSuccess ? 0 : -1;
}
#endif
