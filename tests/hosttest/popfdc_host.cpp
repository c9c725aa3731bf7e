// popfdc_host.cpp -- the per-threshold part of hbvx_population_fdc (hydrodl2_amd/csrc/hbv_pop.h: FdcSlot -- one
// threshold's exceedance count and volume) compiled for the host, one FdcSlot per (threshold, basin) fed day by day as the
// kernel's lanes feed theirs (tests/test_popfdc_host.py; tests/test_population_fdc_gpu.py holds the kernel to it).
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

// y [T,B] the routed flow of every day; enter [T,B] bytes, nonzero where the day enters the curve, or nullptr (every day
// does); thr [K,B].  Out: count [K,B] int32, volume [K,B].  Returns 0, or -1 for K outside 1..FDC_MAX_THR.
extern "C" int popfdc_host(int T, int B, int K, const float *y, const uint8_t *enter, const float *thr, int32_t *count,
                           float *volume)
{
    if (K < 1 || K > FDC_MAX_THR) return -1;
    for (int k = 0; k < K; k++)
        for (int b = 0; b < B; b++) {
            FdcSlot f;
            f.start();
            for (int t = 0; t < T; t++)
                if (!enter || enter[(int64_t)t * B + b]) f.push(y[(int64_t)t * B + b], thr[(int64_t)k * B + b]);
            count[(int64_t)k * B + b] = (int32_t)f.n;
            volume[(int64_t)k * B + b] = f.vol;
        }
    return 0;
}
