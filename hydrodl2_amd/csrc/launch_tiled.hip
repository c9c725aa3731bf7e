// launch_tiled.hip -- host dispatch of the wave-specialised LDS-tiled kernels (hbv_tiled.h).  The forward also serves
// the implicit scheme (launch_adj.hip): there the tiled stepper runs the Newton solve.
#include "hbvx_host.h"
#include "hbv_tiled.h"

using namespace hbvx;
using namespace hbvx_host;

static bool geom_fwd(const hbvx_desc *d, const hbvx_fwd_out *o, TileGeom &g)
{
    g = TileGeom{};
    g.lgMp = lg_members(d->M);
    g.ND = count_dyn(d);
    g.NDm = g.ND + (d->muwts ? 1 : 0);
    const int NF = (d->model == HBVX_MODEL_HBV10) ? 11 : (d->model == HBVX_MODEL_HBVADJ ? 1 : 12);
    // Few workgroups (cfg2: 168 on 256 CUs): deep tiles, one workgroup owns its CU.  Many
    // workgroups (cfg5: 3125): shallow tiles so that several steppers share a CU (LDS decides how
    // many) -- measured at cfg5: Kt 16/8 -> 7.4 ms, Kt 4 -> 5.8 ms.
    const int wgs = (d->B + (64 >> g.lgMp) - 1) / (64 >> g.lgMp);
    const int ktmax = env_int("HBVX_KT", wgs >= 1024 ? 4 : 16);
    for (int Kt = 16; Kt >= 1; Kt >>= 1) {
        if (Kt > ktmax) continue;
        g.Kt = Kt;
        g.off_pin = Kt * 256;
        g.in_sz = Kt * (256 + g.NDm * 64);
        g.off_tout = Kt * 64 * (o->flux ? NF : 0);
        g.out_sz = g.off_tout + Kt * 64 * (o->traj ? TILE_TRAJ_ROWS : 0);
        if (g.out_sz == 0) g.out_sz = 4;
        if (2 * (g.in_sz + g.out_sz) * 4 <= LDS_BUDGET) return true;
    }
    return false;
}

static bool geom_bwd(const hbvx_desc *d, const hbvx_bwd_io *io, TileGeom &g)
{
    g = TileGeom{};
    g.lgMp = lg_members(d->M);
    g.ND = count_dyn(d);
    g.NDm = g.ND + (d->muwts ? 1 : 0);
    const int NF = io->grad_flux ? ((d->model == HBVX_MODEL_HBV10) ? 11 : 12) : 4; // staged series
    const int bpw = 64 >> g.lgMp;
    const int ktmax = env_int("HBVX_KT", 16);
    for (int Kt = 16; Kt >= 1; Kt >>= 1) {
        if (Kt > ktmax) continue;
        g.Kt = Kt;
        g.off_pin = Kt * 256;
        g.off_tin = g.off_pin + Kt * g.NDm * 64;
        g.off_gin = g.off_tin + Kt * TILE_TRAJ_ROWS * 64;
        g.in_sz = (g.off_gin + Kt * NF * bpw + 3) & ~3;
        g.off_xout = Kt * 64 * g.ND;
        g.off_mout = g.off_xout + Kt * 64 * (io->grad_x ? 3 : 0);
        g.out_sz = g.off_mout + Kt * 64 * (io->grad_muwts ? 1 : 0);
        if (g.out_sz == 0) g.out_sz = 4;
        if (2 * (g.in_sz + g.out_sz) * 4 <= LDS_BUDGET) return true;
    }
    return false;
}

// threads of a tiled launch: one stepper wave and nh helper waves (HBVX_NH; the implicit scheme's stepper takes seven
// at every grid size); limit256: the kernel's HBV 2.0 / hourly instances are compiled for 256 threads (hbv_tiled.h,
// bwd_tiled_threads)
static int tiled_threads(const hbvx_desc *d, dim3 grid, bool limit256)
{
    int nh = env_int("HBVX_NH", d->model != HBVX_MODEL_HBVADJ && grid.x >= 1024 ? 3 : 7);
    nh = nh < 1 ? 1 : (nh > 7 ? 7 : nh);
    if (limit256 && (d->model == HBVX_MODEL_HBV20 || d->model == HBVX_MODEL_HOURLY)) nh = nh > 3 ? 3 : nh;
    return 64 * (1 + nh);
}

bool hbvx_host::try_fwd_tiled(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream, int *rc)
{
        FwdTArgs ta;
        if (use_tiled(d) && geom_fwd(d, out, ta.g)) {
            ta.d = *d;
            ta.o = *out;
            const int bpw_t = 64 >> ta.g.lgMp;
            dim3 grid_t((d->B + bpw_t - 1) / bpw_t);
            const size_t lds = (size_t)2 * (ta.g.in_sz + ta.g.out_sz) * 4;
            const bool dyn = ta.g.NDm > 0;
            const int threads = tiled_threads(d, grid_t, false);
            hipStream_t st = (hipStream_t)stream;
            auto launch = [&](auto m, auto be) {
                return dyn ? launch_tiled_one(k_fwd_tiled<m, be, true>, ta, grid_t, threads, lds, st)
                           : launch_tiled_one(k_fwd_tiled<m, be, false>, ta, grid_t, threads, lds, st);
            };
            if (d->model == HBVX_MODEL_HBVADJ) {     // hbvx_adj_forward: no note_dispatch
                hipError_t e = with_adj(d, false, [&](auto be, auto) { return launch(std::integral_constant<int, MODEL_HBVADJ>{}, be); });
                *rc = e != hipSuccess ? hip_fail(e, "hbvx_adj_forward (tiled) launch") : HBVX_OK;
                return true;
            }
            hipError_t e = with_model(d, launch);
            note_dispatch(0, "tiled");
            *rc = e != hipSuccess ? hip_fail(e, "hbvx_forward (tiled) launch") : HBVX_OK;
            return true;
        }
    return false;
}

bool hbvx_host::try_bwd_tiled(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc)
{
        BwdTArgs ta;
        if (use_tiled(d) && geom_bwd(d, io, ta.g)) {
            ta.d = *d;
            ta.io = *io;
            const int bpw_t = 64 >> ta.g.lgMp;
            dim3 grid_t((d->B + bpw_t - 1) / bpw_t);
            const size_t lds = (size_t)2 * (ta.g.in_sz + ta.g.out_sz) * 4;
            const bool dyn = ta.g.NDm > 0, gfull = io->grad_flux != nullptr;
            const int threads = tiled_threads(d, grid_t, dyn);
            hipStream_t st = (hipStream_t)stream;
            store_gate(io, st);
            hipError_t e = with_model(d, [&](auto m, auto be) {
                if (dyn)
                    return gfull ? launch_tiled_one(k_bwd_tiled<m, be, true, true>, ta, grid_t, threads, lds, st)
                                 : launch_tiled_one(k_bwd_tiled<m, be, true, false>, ta, grid_t, threads, lds, st);
                return gfull ? launch_tiled_one(k_bwd_tiled<m, be, false, true>, ta, grid_t, threads, lds, st)
                             : launch_tiled_one(k_bwd_tiled<m, be, false, false>, ta, grid_t, threads, lds, st);
            });
            note_dispatch(1, "tiled");
            *rc = e != hipSuccess ? hip_fail(e, "hbvx_backward (tiled) launch") : HBVX_OK;
            return true;
        }
    return false;
}
