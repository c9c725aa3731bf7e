// step_jg_host.cpp -- TEST HARNESS: one HBV 1.0 day of hbvx::Step (hydrodl2_amd/csrc/hbv_step.h) on the host, its
// parameter-Jacobian application jt_gp<LEVEL, AFF>() next to bwd() and jt_unit / jt_affine on the same vector, so
// tests/test_step_jg_host.py can check the one-pass adjoint's per-vector gp sums without a GPU.  Built only by that
// test; never shipped or loaded by the package.
#include <cstring>

#include "../../hydrodl2_amd/csrc/hbv_step.h"

using namespace hbvx;

namespace {

// level 0 / 1 / 2: a unit-adjoint vector (a[2..4] / a[3..4] zero at levels 0 / 1); level 3: the affine offset with
// the runoff sources src[3] = (gQ0 + gQ, gQ1 + gQ, gQ2 + gQ).
// Out: gp_new / a_new from jt_gp, gp_ref / a_ref from bwd(), a_jt from jt_unit / jt_affine.
template <bool BETAET>
void day(const float *st, const float *p_in, const float *x, float nz, int tie_perc, int level, const float *a_in,
         const float *src, float *gp_new, float *a_new, float *gp_ref, float *a_ref, float *a_jt)
{
    typedef Step<MODEL_HBV10, BETAET> S;
    float p[NPARAM_MAX];
    memcpy(p, p_in, sizeof p);
    S s;
    for (int pass = 0; pass < (tie_perc ? 2 : 1); pass++) {
        if (pass == 1) p[P_PERC] = s.SUZ1;
        s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
        s.P = x[0]; s.Tf = x[1]; s.PET = x[2];
        s.template fwd<false, false>(p, nz, 0.0f, 0.0f, 0.0f, 0.0f);
    }
    const typename S::JT c = s.jt_coef(p, nz);
    const typename S::JG k = s.jg_coef(p, nz);
    for (int i = 0; i < NPARAM_MAX; i++) gp_new[i] = gp_ref[i] = 0.0f;
    memcpy(a_new, a_in, 5 * sizeof(float));
    memcpy(a_jt, a_in, 5 * sizeof(float));
    memcpy(a_ref, a_in, 5 * sizeof(float));
    if (level == 0) { S::template jt_gp<0>(c, k, a_new, gp_new); S::template jt_unit<0>(c, a_jt); }
    if (level == 1) { S::template jt_gp<1>(c, k, a_new, gp_new); S::template jt_unit<1>(c, a_jt); }
    if (level == 2) { S::template jt_gp<2>(c, k, a_new, gp_new); S::template jt_unit<2>(c, a_jt); }
    if (level == 3) {
        S::template jt_gp<2, true>(c, k, a_new, gp_new, src[0], src[1], src[2]);
        S::jt_affine(c, a_jt, src[0], src[1], src[2]);
    }
    FluxGrad g;
    memset(&g, 0, sizeof g);
    if (level == 3) { g.gQ0 = src[0]; g.gQ1 = src[1]; g.gQ2 = src[2]; }
    float gx[3];
    s.bwd(p, nz, g, a_ref, gp_ref, gx);
}

} // namespace

extern "C" int stepjg_day(int betaet, const float *st, const float *p, const float *x, float nz, int tie_perc,
                          int level, const float *a, const float *src, float *gp_new, float *a_new, float *gp_ref,
                          float *a_ref, float *a_jt)
{
    if (betaet) day<true>(st, p, x, nz, tie_perc, level, a, src, gp_new, a_new, gp_ref, a_ref, a_jt);
    else day<false>(st, p, x, nz, tie_perc, level, a, src, gp_new, a_new, gp_ref, a_ref, a_jt);
    return 0;
}
