// gram.hip -- hbvx_gram: per-basin normal equations of the direction-major tangent series (include/hbvx.h).
// The arithmetic, the time slicing and the workspace layout are in hbv_gram.h (shared with the host test); the
// kernels here stage operands and map lanes onto it.  Why lane = basin with register tiles and not MFMA: DESIGN.md.
#include "hbvx_host.h"
#include "hbv_gram.h"

using namespace hbvx_host;
using namespace hbvx_gramk;

namespace {

struct GramArgs {
    Plan p;
    const float *s, *w, *r;
    int64_t series_stride;
    float *ws;
    float *gram, *rhs, *cost;
    int U;      // units = G * S
};

// Pass one.  One workgroup of eight waves per (unit, block pair): unit = (basin group of 64 lanes, time slice), block
// pair = 32 x 32 columns (BI <= BJ).  Per chunk of DAYS days the workgroup stages the 64 columns of its two blocks, the
// weights and the residuals in LDS -- one 16-byte record of four days per (column, lane), so a wave's read of a column
// is one conflict-free ds_read_b128 -- and every wave feeds two 8 x 8 register tiles from them: 66 global rows per day
// serve 1024 multiply-adds per lane (an 8 x 8 tile fed from global memory alone gets 64 from 16, and ran at the speed
// of HBM: profiles/r12_normal_eq.md).  The chunk after the one being summed is in flight in registers meanwhile; two LDS
// buffers, one barrier per chunk.
// Workgroups are dealt to the XCDs round-robin, so eight consecutive block indices go to eight different units and
// the block pairs of a unit follow each other on ONE XCD, reading the same rows at about the same time (speed only;
// nothing depends on placement).
constexpr int GWAVES = 8;                           // waves of a workgroup
constexpr int BCOLS = BLOCK * TILE;                 // 32 columns per block
constexpr int NSTAGE = 2 * BCOLS + 2;               // staged rows: block BI, block BJ, w, r
constexpr int PER_WAVE = (NSTAGE + GWAVES - 1) / GWAVES;

template <bool HAS_W, bool HAS_R>
__global__ void __launch_bounds__(64 * GWAVES) k_gram_partial(const GramArgs A)
{
    __shared__ float4 stage[2][NSTAGE][64];
    const Plan &p = A.p;
    const int id = blockIdx.x;
    const int kk = id >> 3;
    const int unit = (kk / p.NWG) * 8 + (id & 7);
    if (unit >= A.U) return;                        // whole workgroups only: no barrier is left waiting
    const int g = unit % p.G, sl = unit / p.G;
    int BI, BJ;
    workgroup_blocks(p.NB, kk % p.NWG, &BI, &BJ);
    const bool dblock = BI == BJ;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: what hangs on it stays scalar
    const int b = g * 64 + lane;
    const bool store = b < p.B;
    const int bl = store ? b : p.B - 1;
    const int t0 = sl * p.L;
    const int t1 = t0 + p.L < p.T ? t0 + p.L : p.T;

    // the rows this wave stages: row q = wave + GWAVES * m;  q < 32: column BI*32 + q, q < 64: column BJ*32 + q - 32
    // (not staged in a diagonal block: the same columns), 64: w, 65: r
    const float *src[PER_WAVE];
    bool take[PER_WAVE];
#pragma unroll
    for (int m = 0; m < PER_WAVE; m++) {
        const int q = wave + GWAVES * m;
        take[m] = q < NSTAGE;
        const float *base = A.s;
        if (q < 2 * BCOLS) {
            int c = (q < BCOLS ? BI * BCOLS + q : BJ * BCOLS + q - BCOLS);
            c = c < p.C ? c : p.C - 1;
            base = A.s + (int64_t)c * A.series_stride;
            if (q >= BCOLS && dblock) take[m] = false;
        } else if (q == 2 * BCOLS) {
            base = A.w;
            if (!HAS_W) take[m] = false;
        } else {
            base = A.r;
            if (!HAS_R) take[m] = false;
        }
        src[m] = take[m] ? base : A.s;
    }
    float pre[PER_WAVE][DAYS];
    auto fetch = [&](int t) {
        int64_t off[DAYS];
#pragma unroll
        for (int k = 0; k < DAYS; k++) off[k] = (int64_t)(t + k < t1 ? t + k : t1 - 1) * p.B + bl;
#pragma unroll
        for (int m = 0; m < PER_WAVE; m++)
            if (take[m]) {
#pragma unroll
                for (int k = 0; k < DAYS; k++) pre[m][k] = src[m][off[k]];
            }
    };

    // the two tiles of this wave: rows of tile I, columns of tiles J0 and J0 + 1
    const int wi = wave >> 1, wj = (wave & 1) * 2;
    const int I = BI * BLOCK + wi;
    const int rowI = wi * TILE;                                        // staged row of column I*8
    int J[2], rowJ[2];
    bool on[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        J[q] = BJ * BLOCK + wj + q;
        rowJ[q] = (dblock ? 0 : BCOLS) + (wj + q) * TILE;
        on[q] = I < p.NT && J[q] < p.NT && I <= J[q];
    }
    float acc[2][TILE][TILE], rh[TILE], cost = 0.0f;
#pragma unroll
    for (int i = 0; i < TILE; i++) {
        rh[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < TILE; j++) acc[0][i][j] = acc[1][i][j] = 0.0f;
    }

    fetch(t0);
    int buf = 0;
    for (int t = t0; t < t1; t += DAYS, buf ^= 1) {
#pragma unroll
        for (int m = 0; m < PER_WAVE; m++)
            if (take[m]) stage[buf][wave + GWAVES * m][lane] = make_float4(pre[m][0], pre[m][1], pre[m][2], pre[m][3]);
        __syncthreads();
        if (t + DAYS < t1) fetch(t + DAYS);
        if (!(on[0] || on[1])) continue;
        const int nd = t1 - t < DAYS ? t1 - t : DAYS;
        float a[TILE][DAYS], wv[DAYS], rv[DAYS];
        if (HAS_W) {
            const float4 x = stage[buf][2 * BCOLS][lane];
            wv[0] = x.x; wv[1] = x.y; wv[2] = x.z; wv[3] = x.w;
        }
#pragma unroll
        for (int i = 0; i < TILE; i++) {
            const float4 x = stage[buf][rowI + i][lane];
            a[i][0] = HAS_W ? wv[0] * x.x : x.x;
            a[i][1] = HAS_W ? wv[1] * x.y : x.y;
            a[i][2] = HAS_W ? wv[2] * x.z : x.z;
            a[i][3] = HAS_W ? wv[3] * x.w : x.w;
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (!on[q]) continue;
            const bool diag = I == J[q];
#pragma unroll
            for (int j = 0; j < TILE; j++) {
                const float4 x = stage[buf][rowJ[q] + j][lane];
                const float v[DAYS] = {x.x, x.y, x.z, x.w};
                if (diag) column_days<true>(nd, a, v, j, acc[q]);
                else column_days<false>(nd, a, v, j, acc[q]);
            }
            if (HAS_R && diag) {
                const float4 x = stage[buf][2 * BCOLS + 1][lane];
                rv[0] = x.x; rv[1] = x.y; rv[2] = x.z; rv[3] = x.w;
                rhs_days(nd, a, rv, rh);
                if (I == 0) cost_days<HAS_W>(nd, wv, rv, cost);
            }
        }
    }
    if (!store) return;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (!on[q]) continue;
        if (I == J[q]) {
            store_tile<true>(p, A.ws, sl, b, I, J[q], acc[q]);
            if (HAS_R) store_rhs(p, A.ws, sl, b, I, rh, cost);
        } else {
            store_tile<false>(p, A.ws, sl, b, I, J[q], acc[q]);
        }
    }
}

// Pass two, gram: one workgroup per (basin group, tile pair).  Lanes are basins while the slices are summed
// (coalesced workspace rows), then the 64 x 64 block turns through LDS so that the stores run along a matrix row.
__global__ void __launch_bounds__(256) k_gram_reduce(const GramArgs A)
{
    __shared__ float tile[TT][65];
    const Plan &p = A.p;
    const int g = blockIdx.x;
    int I = 0;
    int64_t rest = blockIdx.y;
    for (; I < p.NT - 1 && rest >= p.NT - I; I++) rest -= p.NT - I;
    const int J = I + (int)rest;
    const bool diag = I == J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = g * 64 + lane;
    const int64_t slice_stride = p.NPAIR * TT * p.B;
    for (int ij = wave * (TT / 4); ij < (wave + 1) * (TT / 4); ij++) {
        const bool have = b < p.B && !(diag && (ij / TILE) > (ij % TILE));
        tile[ij][lane] = have ? ordered_sum(A.ws + ws_gram_at(p, 0, blockIdx.y, ij, b), p.S, slice_stride) : 0.0f;
    }
    __syncthreads();
    const int64_t CC = (int64_t)p.C * p.C;
    for (int idx = threadIdx.x; idx < 64 * TT; idx += 256) {
        const int bl = idx / TT, i = (idx % TT) / TILE, j = idx % TILE;
        const int bb = g * 64 + bl, c = I * TILE + i, e = J * TILE + j;
        if (bb < p.B && c < p.C && e < p.C) A.gram[bb * CC + (int64_t)c * p.C + e] = tile[stored_ij(diag, i, j)][bl];
    }
    if (diag) return;
    for (int idx = threadIdx.x; idx < 64 * TT; idx += 256) {       // the mirror block: a copy, i along the row
        const int bl = idx / TT, j = (idx % TT) / TILE, i = idx % TILE;
        const int bb = g * 64 + bl, c = I * TILE + i, e = J * TILE + j;
        if (bb < p.B && c < p.C && e < p.C) A.gram[bb * CC + (int64_t)e * p.C + c] = tile[i * TILE + j][bl];
    }
}

// Pass two, rhs and cost: blockIdx.y = column, C = the cost.
__global__ void __launch_bounds__(64) k_gram_reduce_rhs(const GramArgs A)
{
    const Plan &p = A.p;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int c = blockIdx.y;
    const float *wr = A.ws + ws_gram_floats(p);
    if (c < p.C) A.rhs[(int64_t)b * p.C + c] = ordered_sum(wr + ws_rhs_at(p, 0, c, b), p.S, (int64_t)p.C * p.B);
    else A.cost[b] = ordered_sum(wr + ws_rhs_floats(p) + ws_cost_at(p, 0, b), p.S, p.B);
}

int check(const hbvx_gram_desc *g, const char **msg)
{
    if (!g) { *msg = "hbvx_gram: descriptor is NULL"; return HBVX_E_NULL; }
    if (g->abi_version != HBVX_ABI_VERSION) { *msg = "hbvx_gram: abi_version mismatch"; return HBVX_E_ABI; }
    if (g->T <= 0 || g->B <= 0 || g->C <= 0) { *msg = "hbvx_gram: T/B/C must be positive"; return HBVX_E_SHAPE; }
    if (g->C > HBVX_GRAM_MAX_C) { *msg = "hbvx_gram: C is above HBVX_GRAM_MAX_C"; return HBVX_E_SHAPE; }
    if (g->series_stride < (int64_t)g->T * g->B) { *msg = "hbvx_gram: series_stride is below T*B"; return HBVX_E_SHAPE; }
    return HBVX_OK;
}

} // namespace

extern "C" uint64_t hbvx_gram_workspace_bytes(const hbvx_gram_desc *g)
{
    const char *msg;
    if (check(g, &msg) != HBVX_OK) return 0;
    return (uint64_t)ws_floats(make_plan(g->T, g->B, g->C)) * sizeof(float);
}

extern "C" int hbvx_gram(const hbvx_gram_desc *g, const float *s, const float *w, const float *r, float *gram,
                         float *rhs, float *cost, void *workspace, uint64_t workspace_bytes, void *stream)
{
    const char *msg = "";
    const int rc = check(g, &msg);
    if (rc != HBVX_OK) return fail(rc, msg);
    if (!s) return fail(HBVX_E_NULL, "hbvx_gram: s is NULL");
    if (!gram) return fail(HBVX_E_NULL, "hbvx_gram: gram is NULL");
    if (r && (!rhs || !cost)) return fail(HBVX_E_NULL, "hbvx_gram: rhs / cost is NULL although r is given");
    GramArgs A;
    A.p = make_plan(g->T, g->B, g->C);
    if (!workspace || workspace_bytes < (uint64_t)ws_floats(A.p) * sizeof(float))
        return fail(HBVX_E_NULL, "hbvx_gram: workspace is missing or smaller than hbvx_gram_workspace_bytes()");
    A.s = s; A.w = w; A.r = r;
    A.series_stride = g->series_stride;
    A.ws = (float *)workspace;
    A.gram = gram; A.rhs = rhs; A.cost = cost;
    A.U = A.p.G * A.p.S;
    const int64_t blocks = (int64_t)((A.U + 7) / 8) * 8 * A.p.NWG;
    if (blocks > 0x7fffffffLL) return fail(HBVX_E_SHAPE, "hbvx_gram: problem too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), threads(64 * GWAVES);
    if (w && r) hipLaunchKernelGGL((k_gram_partial<true, true>), grid, threads, 0, st, A);
    else if (w) hipLaunchKernelGGL((k_gram_partial<true, false>), grid, threads, 0, st, A);
    else if (r) hipLaunchKernelGGL((k_gram_partial<false, true>), grid, threads, 0, st, A);
    else hipLaunchKernelGGL((k_gram_partial<false, false>), grid, threads, 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_gram launch (slices)");
    hipLaunchKernelGGL(k_gram_reduce, dim3(A.p.G, (unsigned)A.p.NPAIR), dim3(256), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_gram launch (gram)");
    if (r) {
        hipLaunchKernelGGL(k_gram_reduce_rhs, dim3(A.p.G, A.p.C + 1), dim3(64), 0, st, A);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "hbvx_gram launch (rhs)");
    }
    return HBVX_OK;
}
