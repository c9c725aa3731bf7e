// Host restatement of k_gp_score (hydrodl2_amd/csrc/hbv_gage_pop.h): a [T,G] gage series through hbvx_popk::PeriodMean
// and hbvx_popk::BasinStats::score, one set per gage, hour by hour with the kernel's period cursor.  Built with
// -ffp-contract=off like the library, so the chains are the kernel's operations on the same values.
#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

template <int TR>
static void run(int T, int G, int K, const int *ends, const float *series, const float *target, const float *w,
                const float *shift, const float *eps, float *mean_out, float *mean_t, float *out)
{
    for (int g = 0; g < G; g++) {
        BasinStats bs;
        bs.start(false, shift[g], TR == T_LOG ? eps[g] : 0.0f);
        PeriodMean pm;
        pm.acc = 0.0f;
        int kf = 0, sf = 0, ef = K > 0 ? ends[0] : -1;
        for (int t = 0; t < T && kf < K; t++) {
            pm.add(series[(long)t * G + g], t == sf);
            if (t == ef) {
                const int n = ef - sf + 1;
                const float mean = n == 1 ? pm.acc : pm.close(n);
                bs.score<TR>(mean, target[(long)kf * G + g], w ? w[(long)kf * G + g] : 1.0f);
                if (mean_out) mean_out[(long)kf * G + g] = mean;
                if (mean_t) mean_t[(long)kf * G + g] = bs.transform<TR>(mean);
                kf++;
                sf = t + 1;
                if (kf < K) ef = ends[kf];
            }
        }
        out[0 * G + g] = bs.cost;
        out[1 * G + g] = bs.s1;
        out[2 * G + g] = bs.s2;
        out[3 * G + g] = bs.s3;
    }
}

// series [T,G]; ends [K] closing hours; target / w [K,G] (w may be NULL); shift / eps [G]; mean_out / mean_t [K,G] (the
// period means and their transform, either may be NULL); out [4,G] = sse, s1, s2, s3.  Returns 0, or 1 for a bad transform.
extern "C" int gagepop_host(int T, int G, int K, int transform, const int *ends, const float *series, const float *target,
                            const float *w, const float *shift, const float *eps, float *mean_out, float *mean_t, float *out)
{
    switch (transform) {
    case T_NONE: run<T_NONE>(T, G, K, ends, series, target, w, shift, eps, mean_out, mean_t, out); return 0;
    case T_SQRT: run<T_SQRT>(T, G, K, ends, series, target, w, shift, eps, mean_out, mean_t, out); return 0;
    case T_LOG: run<T_LOG>(T, G, K, ends, series, target, w, shift, eps, mean_out, mean_t, out); return 0;
    default: return 1;
    }
}
