// popperiod_host.cpp -- the per-basin part of hbvx_population_period (hydrodl2_amd/csrc/hbv_pop.h: a BasinStats and an
// AuxStats fed from two PeriodMeans) compiled for the host, one set per basin fed day by day with the cursors of
// k_pop's period form (the same header): tests/test_popperiod_host.py.  Built together with
// popjoint_host.cpp, popstats_host.cpp and pop_host.cpp, whose popjoint_host the test holds the daily calendars to.
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_pop.h"

using namespace hbvx_popk;

namespace {

template <int TR>
void run(int T, int B, int t_first, const float *a, const float *bb, const float *q, const float *target, const float *w,
         const float *shift, const float *eps, const float *v, const float *atarget, const float *aw, const float *ashift,
         int KF, const int *fend, int KA, const int *aend, float *y, float *fmean, float *fmean_t, float *amean,
         float *out, float *aout)
{
    const int L = T < UH ? T : UH;
    for (int b = 0; b < B; b++) {
        BasinStats bs;
        bs.start(a != nullptr, shift[b], TR == T_LOG ? eps[b] : 0.0f);
        if (a) gamma_taps(a[b], bb[b], L, bs.uh);
        AuxStats ax;
        ax.start(ashift[b]);
        PeriodMean pf, pa;
        pf.acc = pa.acc = 0.0f;
        int kf = 0, sf = 0, ef = KF > 0 ? fend[0] : -1;
        int ka = 0, sa = 0, ea = KA > 0 ? aend[0] : -1;
        for (int t = 0; t < T; t++) {
            const float yy = bs.Basin::push(q[(int64_t)t * B + b], 0.0f, 0.0f, false);
            y[(int64_t)t * B + b] = yy;
            const int rel = t - t_first;
            if (rel >= 0 && kf < KF) {
                pf.add(yy, rel == sf);
                if (rel == ef) {
                    const float mean = pf.close(ef - sf + 1);
                    const int64_t row = (int64_t)kf * B + b;
                    bs.score<TR>(mean, target[row], w ? w[row] : 1.0f);
                    fmean[row] = mean;
                    fmean_t[row] = bs.transform<TR>(mean);
                    kf++;
                    sf = rel + 1;
                    if (kf < KF) ef = fend[kf];
                }
            }
            if (rel >= 0 && ka < KA) {
                pa.add(v[(int64_t)t * B + b], rel == sa);
                if (rel == ea) {
                    const float mean = pa.close(ea - sa + 1);
                    const int64_t row = (int64_t)ka * B + b;
                    ax.push(mean, atarget[row], aw ? aw[row] : 1.0f);
                    amean[row] = mean;
                    ka++;
                    sa = rel + 1;
                    if (ka < KA) ea = aend[ka];
                }
            }
        }
        out[0 * B + b] = bs.cost;
        out[1 * B + b] = bs.s1;
        out[2 * B + b] = bs.s2;
        out[3 * B + b] = bs.s3;
        aout[0 * B + b] = ax.sse;
        aout[1 * B + b] = ax.s1;
        aout[2 * B + b] = ax.s2;
        aout[3 * B + b] = ax.s3;
    }
}

} // namespace

// q, v [T,B] the day's un-routed flow and aux value; a / bb [B] or nullptr; target (ALREADY transformed) and w [KF,B],
// atarget and aw [KA,B] per period (w, aw may be nullptr); shift, eps, ashift [B]; fend [KF], aend [KA] the closing days
// relative to t_first.  Out: y [T,B] the routed flow of every day, fmean / fmean_t [KF,B] the flow's period means and
// their transform, amean [KA,B] the aux period means (rows of periods that never close are left alone), out / aout [4,B]
// = sse, s1, s2, s3 of the two terms.  Returns 0, or -1 for an unknown transform.
extern "C" int popperiod_host(int T, int B, int t_first, int transform, int KF, int KA, const float *a, const float *bb,
                              const float *q, const float *target, const float *w, const float *shift, const float *eps,
                              const float *v, const float *atarget, const float *aw, const float *ashift, const int *fend,
                              const int *aend, float *y, float *fmean, float *fmean_t, float *amean, float *out, float *aout)
{
    switch (transform) {
    case T_NONE:
        run<T_NONE>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, KF, fend, KA, aend, y, fmean,
                    fmean_t, amean, out, aout);
        return 0;
    case T_SQRT:
        run<T_SQRT>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, KF, fend, KA, aend, y, fmean,
                    fmean_t, amean, out, aout);
        return 0;
    case T_LOG:
        run<T_LOG>(T, B, t_first, a, bb, q, target, w, shift, eps, v, atarget, aw, ashift, KF, fend, KA, aend, y, fmean,
                   fmean_t, amean, out, aout);
        return 0;
    default: return -1;
    }
}
