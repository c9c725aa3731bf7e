// step_tan_host.cpp -- TEST HARNESS: one day of hbvx::Step (hydrodl2_amd/csrc/hbv_step.h) on the host, its
// tangent tan() and its adjoint bwd() on the same intermediates, so tests/test_step_tangent_host.py can check
// <w, J v> == <J^T w, v> without a GPU.  Built only by that test; never shipped or loaded by the package.
#include <cstring>

#include "../../hydrodl2_amd/csrc/hbv_step.h"

using namespace hbvx;

namespace {

// v = (ds[5], dp[NPARAM_MAX], dx[3]);  w = (a[5], g[12]).
// Out: jv_s[5], jv_f[12] = J v;  jtw_s[5], jtw_p[NPARAM_MAX], jtw_x[3] = J^T w;  prim[5 + 12] = states out, series.
// tie_perc: rerun the day with parPERC = SUZ1 of the first run (a binary-minimum tie, 1/2 each).
template <int MODEL, bool BETAET>
void day(const float *st, const float *p_in, const float *x, float nz, float ac, float elev, int tie_perc,
         const float *ds_in, const float *dp, const float *dx, const float *a_in, const float *g_in,
         float *jv_s, float *jv_f, float *jtw_s, float *jtw_p, float *jtw_x, float *prim)
{
    float p[NPARAM_MAX];
    memcpy(p, p_in, sizeof p);
    Step<MODEL, BETAET> s;
    for (int pass = 0; pass < (tie_perc ? 2 : 1); pass++) {
        if (pass == 1) p[P_PERC] = s.SUZ1;
        s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
        s.P = x[0]; s.Tf = x[1]; s.PET = x[2];
        s.template fwd<false, false>(p, nz, ac, elev, 0.0f, 0.0f);
    }
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
}

} // namespace

// model: 0 HBV 1.0, 1 HBV 1.1p, 2 HBV 2.0.  Returns 0, or -1 for an unknown model.
extern "C" int steptan_day(int model, int betaet, const float *st, const float *p, const float *x, float nz, float ac,
                           float elev, int tie_perc, const float *ds, const float *dp, const float *dx, const float *a,
                           const float *g, float *jv_s, float *jv_f, float *jtw_s, float *jtw_p, float *jtw_x,
                           float *prim)
{
#define HBVX_DAY(M_, B_) day<M_, B_>(st, p, x, nz, ac, elev, tie_perc, ds, dp, dx, a, g, jv_s, jv_f, jtw_s, jtw_p, jtw_x, prim)
    if (model == MODEL_HBV10 && !betaet) HBVX_DAY(MODEL_HBV10, false);
    else if (model == MODEL_HBV10) HBVX_DAY(MODEL_HBV10, true);
    else if (model == MODEL_HBV11P) HBVX_DAY(MODEL_HBV11P, true);
    else if (model == MODEL_HBV20) HBVX_DAY(MODEL_HBV20, true);
    else return -1;
#undef HBVX_DAY
    return 0;
}
