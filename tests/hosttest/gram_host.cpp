// gram_host.cpp -- hbvx_gram's per-lane arithmetic, indexing and slice order (hydrodl2_amd/csrc/hbv_gram.h) compiled
// for the host: the same two passes the kernels of gram.hip run, with the lanes as loops (tests/test_gram_host.py).
// Built with -DGRAM_HOST_MAIN it is a stand-alone program over a few small shapes instead (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../hydrodl2_amd/csrc/hbv_gram.h"

using namespace hbvx_gramk;

namespace {

template <bool HAS_W, bool HAS_R>
void pass_one(const Plan &p, const float *s, int64_t stride, const float *w, const float *r, float *ws)
{
    for (int sl = 0; sl < p.S; sl++)
        for (int g = 0; g < p.G; g++)
            for (int wg = 0; wg < p.NWG; wg++) {
                int BI, BJ;
                workgroup_blocks(p.NB, wg, &BI, &BJ);
                for (int I = BI * BLOCK; I < (BI + 1) * BLOCK && I < p.NT; I++)
                    for (int J = BJ * BLOCK; J < (BJ + 1) * BLOCK && J < p.NT; J++) {
                        if (J < I) continue;                       // a diagonal block keeps its upper tiles
                        for (int lane = 0; lane < 64; lane++) {
                            const int b = g * 64 + lane;
                            const bool store = b < p.B;
                            const int bl = store ? b : p.B - 1;
                            if (I == J) lane_partial<true, HAS_W, HAS_R>(p, s, stride, w, r, ws, sl, bl, store, I, J);
                            else lane_partial<false, HAS_W, HAS_R>(p, s, stride, w, r, ws, sl, bl, store, I, J);
                        }
                    }
            }
}

void pass_two(const Plan &p, const float *ws, bool has_r, float *gram, float *rhs, float *cost)
{
    const int64_t slice_stride = p.NPAIR * TT * p.B;
    for (int I = 0; I < p.NT; I++)
        for (int J = I; J < p.NT; J++) {
            const int64_t pair = pair_index(p.NT, I, J);
            for (int b = 0; b < p.B; b++)
                for (int i = 0; i < TILE; i++)
                    for (int j = 0; j < TILE; j++) {
                        const int c = I * TILE + i, e = J * TILE + j;
                        if (c >= p.C || e >= p.C) continue;
                        const float v = ordered_sum(ws + ws_gram_at(p, 0, pair, stored_ij(I == J, i, j), b), p.S, slice_stride);
                        gram[((int64_t)b * p.C + c) * p.C + e] = v;
                        if (I != J) gram[((int64_t)b * p.C + e) * p.C + c] = v;
                    }
        }
    if (!has_r) return;
    const float *wr = ws + ws_gram_floats(p);
    for (int b = 0; b < p.B; b++) {
        for (int c = 0; c < p.C; c++) rhs[(int64_t)b * p.C + c] = ordered_sum(wr + ws_rhs_at(p, 0, c, b), p.S, (int64_t)p.C * p.B);
        cost[b] = ordered_sum(wr + ws_rhs_floats(p) + ws_cost_at(p, 0, b), p.S, p.B);
    }
}

} // namespace

// s: series c at s + c*stride, [T,B] inside; w, r [T,B] or NULL; gram [B,C,C], rhs [B,C], cost [B].  The workspace is
// NaN before pass one: a word pass two reads and pass one did not write shows.
extern "C" void gram_host(int T, int B, int C, long long stride, const float *s, const float *w, const float *r,
                          float *gram, float *rhs, float *cost)
{
    const Plan p = make_plan(T, B, C);
    std::vector<float> ws((size_t)ws_floats(p), std::numeric_limits<float>::quiet_NaN());
    if (w && r) pass_one<true, true>(p, s, stride, w, r, ws.data());
    else if (w) pass_one<true, false>(p, s, stride, w, r, ws.data());
    else if (r) pass_one<false, true>(p, s, stride, w, r, ws.data());
    else pass_one<false, false>(p, s, stride, w, r, ws.data());
    pass_two(p, ws.data(), r != nullptr, gram, rhs, cost);
}

// out[0..1] = slices, days per slice for (T, B)
extern "C" void gram_host_slices(int T, int B, int *out) { time_slices(T, B, &out[0], &out[1]); }

#ifdef GRAM_HOST_MAIN
int main()
{
    const int shapes[4][3] = {{1, 1, 1}, {5, 3, 7}, {70, 67, 17}, {100, 5, 35}};
    int bad = 0;
    for (const auto &sh : shapes) {
        const int T = sh[0], B = sh[1], C = sh[2];
        std::vector<float> s((size_t)C * T * B), w((size_t)T * B), r((size_t)T * B);
        unsigned x = 12345u;
        auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) / 8388608.0f - 1.0f; };
        for (auto &v : s) v = rnd();
        for (auto &v : w) v = std::fabs(rnd());
        for (auto &v : r) v = rnd();
        std::vector<float> gram((size_t)B * C * C), rhs((size_t)B * C), cost(B);
        gram_host(T, B, C, (long long)T * B, s.data(), w.data(), r.data(), gram.data(), rhs.data(), cost.data());
        double worst = 0.0;
        for (int b = 0; b < B; b++)
            for (int c = 0; c < C; c++)
                for (int e = 0; e < C; e++) {
                    double want = 0.0;
                    for (int t = 0; t < T; t++)
                        want += (double)w[(size_t)t * B + b] * s[((size_t)c * T + t) * B + b] * s[((size_t)e * T + t) * B + b];
                    const double d = std::fabs(gram[((size_t)b * C + c) * C + e] - want);
                    worst = d > worst ? d : worst;
                }
        std::printf("T %d B %d C %d: worst |gram - float64| %.3g\n", T, B, C, worst);
        if (!(worst < 1e-3)) bad = 1;
    }
    return bad;
}
#endif
