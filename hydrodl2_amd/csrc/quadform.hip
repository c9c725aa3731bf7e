// quadform.hip -- hbvx_quadform: q[t,b] = |M_b s[:,t,b]|^2 of the direction-major tangent series (include/hbvx.h).
// The arithmetic, the packed factor and the order of every sum are in hbv_quadform.h (shared with the host test); the
// kernels here map lanes onto it.  Why lane = basin and why the factor form: DESIGN.md.
#include "hbvx_host.h"
#include "hbv_quadform.h"

using namespace hbvx_host;
using namespace hbvx_qfk;

namespace {

struct QuadArgs {
    int T, B, C;
    const float *s, *m;
    int64_t series_stride;
    float *packed;      // the workspace
    float *q;
    int chunks;         // groups of QDAYS days
};

// Pass one: the lower triangle of m [B,C,C] goes to the workspace with the basin innermost.  One workgroup per (basin
// group of 64, factor row e); 64 columns at a time turn through LDS: read along a factor row (c the unit-stride axis),
// stored along the basins.  Only c <= e is read.
__global__ void __launch_bounds__(256) k_quadform_pack(const QuadArgs A)
{
    __shared__ float tile[PACK][PACK_PITCH];
    const int g = blockIdx.x, e = blockIdx.y;
    for (int c0 = 0; c0 <= e; c0 += PACK) {
        for (int i = threadIdx.x; i < PACK * PACK; i += 256) pack_read(A.B, A.C, g, e, c0, i, A.m, tile);
        __syncthreads();
        for (int i = threadIdx.x; i < PACK * PACK; i += 256) pack_write(A.B, g, e, c0, i, tile, A.packed);
        __syncthreads();
    }
}

// Pass two: one wave per (basin group, QDAYS days); the waves of a workgroup take consecutive day groups of ONE basin
// group, so they read the same packed factor rows at about the same time (speed only).
__global__ void __launch_bounds__(256) k_quadform(const QuadArgs A)
{
    const int waves = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: the day offsets stay scalar
    const int chunk = blockIdx.x * waves + wave;
    if (chunk >= A.chunks) return;                  // no barrier in this kernel
    const int b0 = blockIdx.y * 64;
    const unsigned lane = threadIdx.x & 63, last = A.B - 1 - b0;     // last: the group's last basin, >= 0
    const bool store = lane <= last;
    lane_days(A.T, A.B, A.C, A.s, A.series_stride, A.packed, chunk * QDAYS, b0, store ? lane : last, store, A.q);
}

int check(const hbvx_gram_desc *g, const char **msg)
{
    if (!g) { *msg = "hbvx_quadform: descriptor is NULL"; return HBVX_E_NULL; }
    if (g->abi_version != HBVX_ABI_VERSION) { *msg = "hbvx_quadform: abi_version mismatch"; return HBVX_E_ABI; }
    if (g->T <= 0 || g->B <= 0 || g->C <= 0) { *msg = "hbvx_quadform: T/B/C must be positive"; return HBVX_E_SHAPE; }
    if (g->C > HBVX_GRAM_MAX_C) { *msg = "hbvx_quadform: C is above HBVX_GRAM_MAX_C"; return HBVX_E_SHAPE; }
    if (g->series_stride < (int64_t)g->T * g->B) { *msg = "hbvx_quadform: series_stride is below T*B"; return HBVX_E_SHAPE; }
    return HBVX_OK;
}

} // namespace

extern "C" uint64_t hbvx_quadform_workspace_bytes(const hbvx_gram_desc *g)
{
    const char *msg;
    if (check(g, &msg) != HBVX_OK) return 0;
    return (uint64_t)ws_floats(g->B, g->C) * sizeof(float);
}

extern "C" int hbvx_quadform(const hbvx_gram_desc *g, const float *s, const float *m, float *q, void *workspace,
                             uint64_t workspace_bytes, void *stream)
{
    const char *msg = "";
    const int rc = check(g, &msg);
    if (rc != HBVX_OK) return fail(rc, msg);
    if (!s) return fail(HBVX_E_NULL, "hbvx_quadform: s is NULL");
    if (!m) return fail(HBVX_E_NULL, "hbvx_quadform: m is NULL");
    if (!q) return fail(HBVX_E_NULL, "hbvx_quadform: q is NULL");
    if (!workspace || workspace_bytes < (uint64_t)ws_floats(g->B, g->C) * sizeof(float))
        return fail(HBVX_E_NULL, "hbvx_quadform: workspace is missing or smaller than hbvx_quadform_workspace_bytes()");
    QuadArgs A;
    A.T = g->T; A.B = g->B; A.C = g->C;
    A.s = s; A.m = m;
    A.series_stride = g->series_stride;
    A.packed = (float *)workspace;
    A.q = q;
    A.chunks = (g->T + QDAYS - 1) / QDAYS;
    const int G = (g->B + 63) / 64;
    if (G > 65535) return fail(HBVX_E_SHAPE, "hbvx_quadform: problem too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_quadform_pack, dim3(G, g->C), dim3(256), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_quadform launch (pack)");
    // four waves per workgroup share factor rows through L1; a grid too small to fill the chip runs one wave each
    const int waves = (int64_t)G * A.chunks >= 2048 ? 4 : 1;
    hipLaunchKernelGGL(k_quadform, dim3((A.chunks + waves - 1) / waves, G), dim3(64 * waves), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_quadform launch (days)");
    return HBVX_OK;
}
