// uh_tap_host.cpp -- the unit hydrograph's per-tap arithmetic (hydrodl2_amd/csrc/hbv_pop.h: gamma_denom, gamma_tap)
// compiled for the host, put together as k_uh_gamma (hbvx.hip) puts it together -- one value per (basin, tap), the 15
// of a basin summed in ascending k with the zeros from L on, each divided by the sum -- beside gamma_taps, the
// restatement the population kernels run.  tests/test_uh_tap_host.py holds the two to each other.
#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// raw [n][15]: the values before normalisation (zero from L on); uh [n][15]: after
extern "C" void uh_by_taps(int n, const float *a, const float *bb, int L, float *raw, float *uh)
{
    for (int b = 0; b < n; b++) {
        float aa = fmaxf(a[b], 0.0f) + 0.1f;
        float theta = fmaxf(bb[b], 0.0f) + 0.5f;
        float v[UH];
        for (int k = 0; k < UH; k++) v[k] = (k < L) ? gamma_tap(gamma_denom(aa, theta), aa, theta, k) : 0.0f;
        float sum = 0.0f;
        for (int k = 0; k < UH; k++) sum += v[k];
        for (int k = 0; k < UH; k++) {
            raw[b * UH + k] = v[k];
            uh[b * UH + k] = (k < L) ? v[k] / sum : 0.0f;
        }
    }
}

extern "C" void uh_by_gamma_taps(int n, const float *a, const float *bb, int L, float *uh)
{
    for (int b = 0; b < n; b++) {
        float w[UH];
        gamma_taps(a[b], bb[b], L, w);
        for (int k = 0; k < UH; k++) uh[b * UH + k] = w[k];
    }
}
