// quadform_host.cpp -- hbvx_quadform's per-lane arithmetic, packed-factor indexing and tiling
// (hydrodl2_amd/csrc/hbv_quadform.h) compiled for the host: the two passes the kernels of quadform.hip run, with the
// lanes as loops (tests/test_quadform_host.py).  Built with -DQUADFORM_HOST_MAIN it is a stand-alone program over a
// few small shapes instead (for a sanitizer build).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../hydrodl2_amd/csrc/hbv_quadform.h"

using namespace hbvx_qfk;

// s: series c at s + c*stride, [T,B] inside; m [B,C,C] (lower triangle read); q [T,B].  The workspace is NaN before
// pass one: a word pass two reads and pass one did not write shows.
extern "C" void quadform_host(int T, int B, int C, long long stride, const float *s, const float *m, float *q)
{
    std::vector<float> ws((size_t)ws_floats(B, C), std::numeric_limits<float>::quiet_NaN());
    const int G = (B + 63) / 64;
    for (int g = 0; g < G; g++)                                     // pass one: one workgroup per (g, e)
        for (int e = 0; e < C; e++) {
            float tile[PACK][PACK_PITCH];                           // stale between turns, as LDS is
            for (int c0 = 0; c0 <= e; c0 += PACK) {
                for (int i = 0; i < PACK * PACK; i++) pack_read(B, C, g, e, c0, i, m, tile);
                for (int i = 0; i < PACK * PACK; i++) pack_write(B, g, e, c0, i, tile, ws.data());
            }
        }
    const int chunks = (T + QDAYS - 1) / QDAYS;
    for (int g = 0; g < G; g++)                                     // pass two: one wave per (g, chunk)
        for (int chunk = 0; chunk < chunks; chunk++)
            for (int lane = 0; lane < 64; lane++) {
                const int b0 = g * 64, last = B - 1 - b0;
                const bool store = lane <= last;
                lane_days(T, B, C, s, stride, ws.data(), chunk * QDAYS, b0, store ? lane : last, store, q);
            }
}

// The definition itself: the two chains of one (t, b), nothing tiled, m read where it lies.
extern "C" void quadform_direct(int T, int B, int C, long long stride, const float *s, const float *m, float *q)
{
    for (int t = 0; t < T; t++)
        for (int b = 0; b < B; b++) {
            float acc = 0.0f;
            for (int e = 0; e < C; e++) {
                float y = 0.0f;
                for (int c = 0; c <= e; c++)
                    y = __builtin_fmaf(m[((size_t)b * C + e) * C + c], s[(size_t)c * stride + (size_t)t * B + b], y);
                acc = __builtin_fmaf(y, y, acc);
            }
            q[(size_t)t * B + b] = acc;
        }
}

#ifdef QUADFORM_HOST_MAIN
int main()
{
    const int shapes[5][3] = {{1, 1, 1}, {5, 3, 7}, {9, 65, 9}, {33, 67, 17}, {12, 5, 70}};
    int bad = 0;
    for (const auto &sh : shapes) {
        const int T = sh[0], B = sh[1], C = sh[2];
        std::vector<float> s((size_t)C * T * B), m((size_t)B * C * C), q((size_t)T * B), d((size_t)T * B);
        unsigned x = 12345u;
        auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) / 8388608.0f - 1.0f; };
        for (auto &v : s) v = rnd();
        for (int b = 0; b < B; b++)
            for (int e = 0; e < C; e++)
                for (int c = 0; c < C; c++)
                    m[((size_t)b * C + e) * C + c] = c <= e ? rnd() : std::numeric_limits<float>::quiet_NaN();
        quadform_host(T, B, C, (long long)T * B, s.data(), m.data(), q.data());
        quadform_direct(T, B, C, (long long)T * B, s.data(), m.data(), d.data());
        int differ = 0;
        for (size_t i = 0; i < q.size(); i++) differ += !(q[i] == d[i] && q[i] >= 0.0f);
        std::printf("T %d B %d C %d: %d of %zu elements differ from the direct chains\n", T, B, C, differ, q.size());
        if (differ) bad = 1;
    }
    return bad;
}
#endif
