// adj_tan_host.cpp -- the implicit scheme's day-level tangent (adj_tanstep) and adjoint (adj_backstep) of
// hydrodl2_amd/csrc/hbv_adj_step.h compiled for the host, one lane-day per row (tests/test_adj_tanstep_host.py).
// Built with -DADJ_TAN_MAIN it is a stand-alone program over a few fixed lane-days instead (for a sanitizer build).
#include <cmath>
#include <cstdio>

#include "../../hydrodl2_amd/csrc/hbv_step.h"
#include "../../hydrodl2_amd/csrc/hbv_adj_step.h"

using namespace hbvx;

namespace {

constexpr int NPH = 13;   // physical parameters per row (slot order; BETAET last, unused without it)

void load_p(const float *src, float *p)
{
    for (int i = 0; i < NPARAM_MAX; i++) p[i] = i < NPH ? src[i] : 0.0f;
}

template <bool BETAET>
void tan_rows(int n, const float *p, const float *clim, const float *x, const float *xt_dot, const float *p_dot,
              const float *c_dot, float *x_dot, float *q_dot)
{
    for (int r = 0; r < n; r++) {
        float pp[NPARAM_MAX], pd[NPARAM_MAX];
        load_p(p + r * NPH, pp);
        load_p(p_dot + r * NPH, pd);
        AdjStep<BETAET> s;
        s.P = clim[r * 3]; s.Tf = clim[r * 3 + 1]; s.PET = clim[r * 3 + 2];
        adj_tanstep<BETAET>(s, pp, x + r * 5, 1.0f, xt_dot + r * 5, pd, c_dot + r * 3, x_dot + r * 5, q_dot[r]);
    }
}

template <bool BETAET>
void back_rows(int n, const float *p, const float *clim, const float *x, const float *gq, float *a, float *gp)
{
    for (int r = 0; r < n; r++) {
        float pp[NPARAM_MAX], g[NPARAM_MAX];
        load_p(p + r * NPH, pp);
        for (int i = 0; i < NPARAM_MAX; i++) g[i] = 0.0f;
        AdjStep<BETAET> s;
        s.P = clim[r * 3]; s.Tf = clim[r * 3 + 1]; s.PET = clim[r * 3 + 2];
        adj_backstep<BETAET>(s, pp, x + r * 5, 1.0f, gq[r], a + r * 5, g);
        for (int i = 0; i < NPH; i++) gp[r * NPH + i] = g[i];
    }
}

} // namespace

// rows: p, p_dot, gp [n,13]; clim, c_dot [n,3]; x, xt_dot, x_dot, a [n,5]; q_dot, gq [n].  dt = 1.
extern "C" void adj_tan_rows(int betaet, int n, const float *p, const float *clim, const float *x,
                             const float *xt_dot, const float *p_dot, const float *c_dot, float *x_dot, float *q_dot)
{
    if (betaet) tan_rows<true>(n, p, clim, x, xt_dot, p_dot, c_dot, x_dot, q_dot);
    else tan_rows<false>(n, p, clim, x, xt_dot, p_dot, c_dot, x_dot, q_dot);
}

// a [n,5]: in dL/dx from the future, out dL/dx_t; gp [n,13]: out
extern "C" void adj_back_rows(int betaet, int n, const float *p, const float *clim, const float *x, const float *gq,
                              float *a, float *gp)
{
    if (betaet) back_rows<true>(n, p, clim, x, gq, a, gp);
    else back_rows<false>(n, p, clim, x, gq, a, gp);
}

#ifdef ADJ_TAN_MAIN
int main()
{
    // a wet warm day, a cold day with an empty snowpack, a dry soil below its clamp
    const float p[3 * NPH] = {
        2.0f, 200.0f, 0.3f, 0.1f, 0.05f, 0.6f, 3.0f, 20.0f, 0.0f, 3.0f, 0.05f, 0.1f, 1.5f,
        4.0f, 120.0f, 0.5f, 0.2f, 0.01f, 0.9f, 1.0f, 5.0f, 1.0f, 5.0f, 0.02f, 0.15f, 0.8f,
        1.2f, 600.0f, 0.1f, 0.05f, 0.1f, 0.3f, 8.0f, 60.0f, -1.0f, 1.0f, 0.08f, 0.05f, 3.0f};
    const float clim[9] = {12.0f, 6.0f, 3.0f, 4.0f, -5.0f, 0.2f, 0.0f, 15.0f, 6.0f};
    const float x[15] = {5.0f, 1.0f, 250.0f, 30.0f, 40.0f, 0.0f, 0.0f, 60.0f, 2.0f, 10.0f, 0.0f, 0.0f, -1.0f, 0.0f, 1.0f};
    float xt_dot[15], p_dot[3 * NPH], c_dot[9], x_dot[15], q_dot[3], gq[3], a[15], gp[3 * NPH];
    for (int i = 0; i < 15; i++) { xt_dot[i] = 0.1f * (float)(i % 7) - 0.3f; a[i] = 0.2f * (float)(i % 5) - 0.4f; }
    for (int i = 0; i < 3 * NPH; i++) p_dot[i] = 0.05f * (float)(i % 9) - 0.2f;
    for (int i = 0; i < 9; i++) c_dot[i] = 0.0f;
    for (int i = 0; i < 3; i++) gq[i] = 0.5f + (float)i;
    double worst = 0.0;
    for (int be = 0; be < 2; be++) {
        float ain[15];
        for (int i = 0; i < 15; i++) ain[i] = a[i];
        adj_tan_rows(be, 3, p, clim, x, xt_dot, p_dot, c_dot, x_dot, q_dot);
        adj_back_rows(be, 3, p, clim, x, gq, ain, gp);
        for (int r = 0; r < 3; r++) {
            double lhs = (double)gq[r] * q_dot[r], rhs = 0.0, mag = std::fabs(lhs);
            for (int k = 0; k < 5; k++) {
                lhs += (double)a[r * 5 + k] * x_dot[r * 5 + k];
                rhs += (double)ain[r * 5 + k] * xt_dot[r * 5 + k];
                mag += std::fabs((double)a[r * 5 + k] * x_dot[r * 5 + k]) + std::fabs((double)ain[r * 5 + k] * xt_dot[r * 5 + k]);
            }
            for (int i = 0; i < (be ? 13 : 12); i++) {
                rhs += (double)gp[r * NPH + i] * p_dot[r * NPH + i];
                mag += std::fabs((double)gp[r * NPH + i] * p_dot[r * NPH + i]);
            }
            const double rel = std::fabs(lhs - rhs) / (1.1920929e-7 * mag);
            worst = rel > worst ? rel : worst;
            std::printf("betaet %d row %d: <a,x_dot>+gQ Q_dot %.7g  <a_t,xt_dot>+<gp,p_dot> %.7g  (%.2f eps)\n", be, r, lhs,
                        rhs, rel);
        }
    }
    return worst < 8.0 ? 0 : 1;
}
#endif
