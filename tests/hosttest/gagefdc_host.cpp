// gagefdc_host.cpp -- the rules of include/hbvx_gage_fdc.h compiled for the host, on one candidate's series [T,G]
// (tests/test_gage_fdc_host.py; tests/test_hourly_fdc_gpu.py holds the kernels to it):
//   gagefdc_host     hbvx_gage_population_fdc: one hbvx_popk::FdcSlot (hydrodl2_amd/csrc/hbv_pop.h) per (level, gage), fed
//                    the scored hours in ascending order as a lane of k_gp_fdc feeds its own;
//   gagequant_host   hbvx_gage_population_quantiles by a plain std::sort of the scored flows -- NOT the kernel's keys and
//                    network, so that it is an oracle of them;
//   gagequant_keys   hbvx_popk::quant_key / quant_value on n values, for the test of the key order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// series [T,G], scored [T,G] (non-zero: the hour enters), thr [K,G].  Out: count [K,G] int32, volume [K,G] float32.
// Returns 0, or -1 for T, G or K < 1.
extern "C" int gagefdc_host(int T, int G, int K, const float *series, const uint8_t *scored, const float *thr,
                            int32_t *count, float *volume)
{
    if (T < 1 || G < 1 || K < 1) return -1;
    for (int k = 0; k < K; k++)
        for (int g = 0; g < G; g++) {
            FdcSlot slot;
            slot.start();
            for (int t = 0; t < T; t++)
                if (scored[(int64_t)t * G + g]) slot.push(series[(int64_t)t * G + g], thr[(int64_t)k * G + g]);
            count[(int64_t)k * G + g] = (int32_t)slot.n;
            volume[(int64_t)k * G + g] = slot.vol;
        }
    return 0;
}

// series, scored as above, rank [K,G].  Out: quantile [K,G].  Returns 0, or -1 for T, G or K < 1.
extern "C" int gagequant_host(int T, int G, int K, const float *series, const uint8_t *scored, const int32_t *rank,
                              float *quantile)
{
    if (T < 1 || G < 1 || K < 1) return -1;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> v;
    for (int g = 0; g < G; g++) {
        v.clear();
        bool any_nan = false;
        for (int t = 0; t < T; t++)
            if (scored[(int64_t)t * G + g]) {
                const float y = series[(int64_t)t * G + g];
                any_nan = any_nan || std::isnan(y);
                v.push_back(y);
            }
        // descending; of two zeros +0 comes first
        if (!any_nan)
            std::sort(v.begin(), v.end(), [](float a, float b) { return a > b || (a == b && !std::signbit(a) && std::signbit(b)); });
        const int64_t n = (int64_t)v.size();
        for (int k = 0; k < K; k++) {
            const int64_t r = rank[(int64_t)k * G + g];
            quantile[(int64_t)k * G + g] = (any_nan || r < 0 || r >= n) ? nan : v[r];
        }
    }
    return 0;
}

extern "C" void gagequant_keys(int n, const float *y, uint32_t *key, float *back)
{
    for (int i = 0; i < n; i++) {
        key[i] = quant_key(y[i]);
        back[i] = quant_value(key[i]);
    }
}
