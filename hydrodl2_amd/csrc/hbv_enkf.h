// hbv_enkf.h -- the arithmetic of hbvx_enkf_update (include/hbvx_enkf.h), one element at a time, compiled by hipcc for
// the device (enkf.hip) and by g++ for the CPU tier (tests/hosttest/enkf_host.cpp).  Both builds run without contraction
// (-ffp-contract=off), every operation below is a correctly rounded float64 add, multiply, divide or square root, and the
// order of every sum is the particle order -- so the same text gives the same bits on both sides.
//
// One call of `element` owns the P values of ONE element e of ONE array: it reads y[:,b] of the element's basin and the
// element's column, and stores the column.  Nothing else is read or written, which is what makes a basin's outputs
// independent of B, the other basins, the other arrays and the launch split, and what allows out == in.
//
// The expressions, parenthesised as evaluated (P, o, R, e_p, x_p, y_p widened to float64 first; `/ P` and `/ (P - 1)` divide
// by the integer widened to float64):
//
//   pass 1   sy = 0;  sy = sy + y_p  (p = 0 .. P-1);           ybar = sy / P
//   pass 2   dy_p = y_p - ybar
//            sv = sv + dy_p * dy_p;                            v = sv / (P - 1);   s = v + R
//            sc = sc + x_p * dy_p;                             c = sc / (P - 1);   K = c / s
//            sx = sx + x_p       (method 1, or rho != 1);      xbar = sx / P
//            se = se + e_p       (method 0);                   ebar = se / P
//            d = (o + ebar) - ybar  (method 0),  o - ybar  (method 1)
//   pass 3   method 0:   xa = x_p + K * ((o + e_p) - y_p)
//            method 1:   alpha = 1 / (1 + sqrt(R / s));  aK = alpha * K;  m = xbar + K * d
//                        xa = m + ((x_p - xbar) - aK * dy_p)
//            rho != 1:   m = xbar + K * d;  xa = m + rho * (xa - m)         (instance INFL; rho == 1 runs the instance
//                                                                            without these operations)
//            xa = xa < lo ? lo : xa;   out = (float)xa
//   pass 3 runs twice: once to see whether every xa and every (float)xa is finite, storing nothing, then to store -- with
//   out == in a column cannot be put back once it is half written.  A column that fails is copied (status 3).
//
// Status precedence (the first that holds): 1 inactive or o NaN (y is not read); 2 R not finite or <= 0, or ybar, v, s
// not finite, or under method 0 an e_p not finite; 3 a non-finite K, xa or (float)xa in this element; 0.  Basins of status
// 1 or 2 are copied.  The thread of a basin's first element in the call's first array (`lead`) stores stats and a status
// of 1 or 2; a 3 is stored by whoever finds it; status is zero before the launch (the launcher clears it).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define HBVX_ENKF_HD __host__ __device__ __forceinline__
#else
#define HBVX_ENKF_HD inline
#endif

namespace hbvx_enkfk {

struct Args {
    int P, B, method;       // method 0: perturbed observations, 1: square root
    double rho;
    const float *y;         // particle p of basin b at y[p * ys + b]
    int64_t ys;
    const float *obs, *obs_var;
    const uint8_t *active;  // or nullptr
    const float *eps;       // [P,B]; method 0
    int *status;            // or nullptr
    double *stats;          // [3,B] or nullptr
    const float *in;        // the array: particle p of element e at in[p * n + e]
    float *out;
    int64_t n;
    int M;
    double lo;
    int64_t e0, count;      // this launch takes elements e0 .. e0 + count - 1
    int lead;               // this array's threads store stats and the statuses 1 and 2
};

HBVX_ENKF_HD bool finite64(double a) { return __builtin_fabs(a) <= 1.7976931348623157e308; }     // false for NaN
HBVX_ENKF_HD bool finite32(float a) { return __builtin_fabsf(a) <= 3.40282347e38f; }

// what pass 3 needs of an element
struct Gain {
    double ybar, o, K, aK, xbar, m, rho, lo;
};

template <bool INFL>
HBVX_ENKF_HD double analysed(int method, const Gain &g, double x, double y, double e)
{
    double xa;
    if (method == 0) xa = x + g.K * ((g.o + e) - y);
    else xa = g.m + ((x - g.xbar) - g.aK * (y - g.ybar));
    if (INFL) xa = g.m + g.rho * (xa - g.m);
    return xa < g.lo ? g.lo : xa;
}

template <bool INFL>
HBVX_ENKF_HD void element(const Args &A, int64_t e)
{
    const int P = A.P, b = (int)((e / A.M) % A.B);
    const bool leader = A.lead && e == (int64_t)b * A.M;
    const float *x = A.in + e, *y = A.y + b, *ep = A.method == 0 ? A.eps + b : nullptr;
    float *xo = A.out + e;
    const int64_t n = A.n, ys = A.ys;
    const double nan = __builtin_nan("");
    int status = 0;
    double ybar = nan, v = nan, d = nan;
    Gain g;
    g.o = nan;
    if (A.active && !A.active[b]) status = 1;
    else {
        g.o = (double)A.obs[b];
        if (g.o != g.o) status = 1;
    }
    if (!status) {
        const double R = (double)A.obs_var[b];
        double sy = 0.0;
#pragma unroll 4
        for (int p = 0; p < P; p++) sy = sy + (double)y[p * ys];
        ybar = sy / (double)P;
        double sv = 0.0, sc = 0.0, sx = 0.0, se = 0.0;
        bool efin = true;
#pragma unroll 4
        for (int p = 0; p < P; p++) {
            const double xp = (double)x[p * n], dy = (double)y[p * ys] - ybar;
            sv = sv + dy * dy;
            sc = sc + xp * dy;
            if (INFL || A.method != 0) sx = sx + xp;
            if (A.method == 0) {
                const double e_p = (double)ep[(int64_t)p * A.B];
                efin = efin && finite64(e_p);
                se = se + e_p;
            }
        }
        v = sv / (double)(P - 1);
        const double s = v + R;
        if (!(finite64(R) && R > 0.0) || !finite64(ybar) || !finite64(v) || !finite64(s) || !efin) status = 2;
        else {
            d = A.method == 0 ? (g.o + se / (double)P) - ybar : g.o - ybar;
            g.ybar = ybar;
            g.K = (sc / (double)(P - 1)) / s;
            g.xbar = sx / (double)P;
            g.aK = A.method == 0 ? 0.0 : (1.0 / (1.0 + __builtin_sqrt(R / s))) * g.K;
            g.m = (INFL || A.method != 0) ? g.xbar + g.K * d : 0.0;
            g.rho = A.rho;
            g.lo = A.lo;
            bool ok = finite64(g.K);
            if (ok) {
#pragma unroll 4
                for (int p = 0; p < P; p++) {
                    const double xa = analysed<INFL>(A.method, g, (double)x[p * n], (double)y[p * ys],
                                                     A.method == 0 ? (double)ep[(int64_t)p * A.B] : 0.0);
                    ok = ok && finite64(xa) && finite32((float)xa);
                }
            }
            if (ok) {
#pragma unroll 4
                for (int p = 0; p < P; p++)
                    xo[p * n] = (float)analysed<INFL>(A.method, g, (double)x[p * n], (double)y[p * ys],
                                                      A.method == 0 ? (double)ep[(int64_t)p * A.B] : 0.0);
            } else {
                status = 3;
                if (A.status) A.status[b] = 3;
            }
        }
    }
    if (status && xo != x) {
#pragma unroll 4
        for (int p = 0; p < P; p++) xo[p * n] = x[p * n];
    }
    if (leader) {
        if (A.status && (status == 1 || status == 2)) A.status[b] = status;
        if (A.stats) {
            A.stats[b] = ybar;
            A.stats[(int64_t)A.B + b] = v;
            A.stats[2 * (int64_t)A.B + b] = d;
        }
    }
}

// the instance of the call's inflation: rho == 1 runs the form that has no inflation in it
HBVX_ENKF_HD void element_of(const Args &A, int64_t e)
{
    if (A.rho != 1.0) element<true>(A, e);
    else element<false>(A, e);
}

} // namespace hbvx_enkfk
