// step_tan_hourly_host.cpp -- TEST HARNESS: one hour of hbvx::Step<MODEL_HOURLY> (hydrodl2_amd/csrc/hbv_step_hourly.h)
// on the host, its tangent tan() and its adjoint bwd() on the same intermediates, so
// tests/test_step_tangent_hourly_host.py can check <w, J v> == <J^T w, v> without a GPU.  Built only by that test;
// never shipped or loaded by the package.
#include <cmath>
#include <cstring>

#include "../../hydrodl2_amd/csrc/hbv_step.h"

using namespace hbvx;

namespace {

typedef Step<MODEL_HOURLY, true> HourStep;

void run(HourStep &s, const float *st, const float *p, const float *x, float nz, float ac, float elev)
{
    s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
    s.P = x[0]; s.Tf = x[1]; s.PET = x[2];
    s.fwd<false>(p, nz, ac, elev, 0.0f, 0.0f);
}

} // namespace

// v = (ds[5], dp[NPARAM_MAX], dx[3]);  w = (a[5], g[12]).
// Out: jv_s[5], jv_f[12] = J v;  jtw_s[5], jtw_p[NPARAM_MAX], jtw_x[3] = J^T w;  prim[5 + 12] = states out, series.
// mode bit 0: rerun the hour with parPERC * dt == SUZ1 of the first run (a binary-minimum tie, 1/2 each); the
// product is rounded, so the parameter is searched among the neighbours of SUZ1 / dt.
// mode bit 1: rerun the hour as a storm: rain at 1.25 x the infiltration capacity of the first run (IE > 0).
// Returns the bits that were reached (bit 0: pdt == SUZ1, bit 1: IE > 0).
extern "C" int steptan_hour(const float *st, const float *p_in, const float *x_in, float nz, float ac, float elev,
                            int mode, const float *ds_in, const float *dp, const float *dx, const float *a_in,
                            const float *g_in, float *jv_s, float *jv_f, float *jtw_s, float *jtw_p, float *jtw_x,
                            float *prim)
{
    float p[NPARAM_MAX], x[3];
    memcpy(p, p_in, sizeof p);
    memcpy(x, x_in, sizeof x);
    HourStep s;
    run(s, st, p, x, nz, ac, elev);
    int reached = 0;
    if (mode & 2) {
        x[0] = (s.fcap * 1.25f + 1.0f) * HourStep::dt_();
        if (!(x[1] >= s.TTe + 1.0f)) x[1] = s.TTe + 1.0f;
        run(s, st, p, x, nz, ac, elev);
    }
    if (mode & 1) {
        const float want = s.SUZ1;
        float c = want / HourStep::dt_();
        for (int i = 0; i < 8; i++) c = nextafterf(c, 0.0f);
        for (int i = 0; i < 17; i++) {
            if (c * HourStep::dt_() == want) {
                p[P_PERC] = c;
                break;
            }
            c = nextafterf(c, INFINITY);
        }
        run(s, st, p, x, nz, ac, elev);
    }
    if (s.pdt == s.SUZ1) reached |= 1;
    if (s.IE > 0.0f) reached |= 2;

    float ds[5];
    memcpy(ds, ds_in, sizeof ds);
    FluxTan f;
    s.tan(p, nz, dp, dx, ds, f);
    memcpy(jv_s, ds, sizeof ds);
    const float fv[12] = {f.Q, f.Q0, f.Q1, f.Q2, f.ET, f.SWE, f.rech, f.exc, f.ef, f.tosoil, f.PERC, f.cap};
    memcpy(jv_f, fv, sizeof fv);

    FluxGrad g;
    g.gQ = g_in[0]; g.gQ0 = g_in[1]; g.gQ1 = g_in[2]; g.gQ2 = g_in[3]; g.gET = g_in[4]; g.gSWE = g_in[5];
    g.grech = g_in[6]; g.gexc = g_in[7]; g.gef = g_in[8]; g.gtosoil = g_in[9]; g.gPERC = g_in[10]; g.gcap = g_in[11];
    float a[5];
    memcpy(a, a_in, sizeof a);
    for (int i = 0; i < NPARAM_MAX; i++) jtw_p[i] = 0.0f;
    s.bwd(p, nz, g, a, jtw_p, jtw_x);
    memcpy(jtw_s, a, sizeof a);

    const float pr[17] = {s.SP3, s.MW3, s.SM4, s.SUZ4, s.SLZ2, s.Q, s.Q0, s.Q1, s.Q2, s.ET, s.SP3, s.rech, s.exc,
                          s.ef, s.tosoil, s.PERC, s.cap};
    memcpy(prim, pr, sizeof pr);
    return reached;
}
