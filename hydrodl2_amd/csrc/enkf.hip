// enkf.hip -- hbvx_enkf_update (include/hbvx_enkf.h): the analysis step of an ensemble Kalman filter over particle arrays.
// The arithmetic and the order of every sum are in hbv_enkf.h (shared with the host test); the kernel maps one thread onto
// one element of an array, threads along the contiguous element index, so the loads of one particle are coalesced and the
// P loads of y[:,b] are one address across a basin's member lanes.  Why a thread owns an element's whole column and why
// the column is streamed and not kept in registers: DESIGN.md.
#include "hbvx_host.h"
#include "../../include/hbvx_enkf.h"
#include "hbv_enkf.h"

#include <cmath>

using namespace hbvx_host;
using namespace hbvx_enkfk;

namespace {

const int THREADS = 256;
const int64_t PIECE = (int64_t)1 << 30;     // elements of one launch: 2^22 workgroups, 2^30 threads

template <bool INFL>
__global__ void __launch_bounds__(THREADS) k_enkf(const Args A)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < A.count) element<INFL>(A, A.e0 + i);
}

int refuse(int code, const char *msg)
{
    static thread_local char buf[160];
    snprintf(buf, sizeof buf, "hbvx_enkf_update: %s", msg);
    return fail(code, buf);
}

// whether [a, a + na) and [b, b + nb) floats share an address
bool overlap(const float *a, int64_t na, const float *b, int64_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

} // namespace

extern "C" uint64_t hbvx_enkf_sizeof(int which)
{
    return which == 0 ? sizeof(hbvx_enkf) : which == 1 ? sizeof(hbvx_enkf_array) : 0;
}

extern "C" int hbvx_enkf_update(const hbvx_enkf *e, void *stream)
{
    if (!e) return refuse(HBVX_E_NULL, "e is NULL");
    if (e->P < 2) return refuse(HBVX_E_SHAPE, "P must be at least 2");
    if (e->B < 1) return refuse(HBVX_E_SHAPE, "B must be at least 1");
    if (e->n_arrays < 1 || e->n_arrays > HBVX_ENKF_MAX_ARRAYS) return refuse(HBVX_E_SHAPE, "n_arrays must be in 1..4");
    if (e->method != HBVX_ENKF_PERTURBED && e->method != HBVX_ENKF_SQRT)
        return refuse(HBVX_E_UNSUPPORTED, "method must be 0 (perturbed observations) or 1 (square root)");
    if (!std::isfinite(e->inflation) || !(e->inflation > 0.0)) return refuse(HBVX_E_SHAPE, "inflation must be finite and > 0");
    if (!e->y) return refuse(HBVX_E_NULL, "y is NULL");
    if (e->y_stride < e->B) return refuse(HBVX_E_SHAPE, "y_stride is below B");
    if (!e->obs) return refuse(HBVX_E_NULL, "obs is NULL");
    if (!e->obs_var) return refuse(HBVX_E_NULL, "obs_var is NULL");
    if (e->method == HBVX_ENKF_PERTURBED && !e->eps) return refuse(HBVX_E_NULL, "eps is NULL under method 0");
    const int64_t ny = (int64_t)(e->P - 1) * e->y_stride + e->B;
    for (int i = 0; i < e->n_arrays; i++) {
        const hbvx_enkf_array &a = e->a[i];
        if (!a.in) return refuse(HBVX_E_NULL, "an array's in is NULL");
        if (!a.out) return refuse(HBVX_E_NULL, "an array's out is NULL");
        if (a.M < 1 || a.n < 1 || a.n % ((int64_t)e->B * a.M) != 0)
            return refuse(HBVX_E_SHAPE, "an array's n must be a positive multiple of B*M, M >= 1");
        if (a.lo != a.lo) return refuse(HBVX_E_SHAPE, "an array's lo is NaN");
        const int64_t na = (int64_t)e->P * a.n;
        if (a.out != a.in && overlap(a.out, na, a.in, na)) return refuse(HBVX_E_SHAPE, "an array's out overlaps its in (only out == in is allowed)");
        if (overlap(a.out, na, e->y, ny)) return refuse(HBVX_E_SHAPE, "an array's out overlaps y");
        for (int j = 0; j < e->n_arrays; j++) {
            if (j == i) continue;
            const int64_t nb = (int64_t)e->P * e->a[j].n;
            if (e->a[j].in && overlap(a.out, na, e->a[j].in, nb)) return refuse(HBVX_E_SHAPE, "an array's out overlaps another array's in");
            if (e->a[j].out && overlap(a.out, na, e->a[j].out, nb)) return refuse(HBVX_E_SHAPE, "an array's out overlaps another array's out");
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (e->status) {
        hipError_t err = hipMemsetAsync(e->status, 0, sizeof(int32_t) * (size_t)e->B, st);
        if (err != hipSuccess) return hip_fail(err, "hbvx_enkf_update clearing status");
    }
    // HBVX_ENKF_PIECE: a smaller piece, for the test that a launch split changes no bit
    int64_t piece = env_int("HBVX_ENKF_PIECE", 0);
    piece = piece > 0 ? (piece + THREADS - 1) / THREADS * THREADS : PIECE;
    if (piece > PIECE) piece = PIECE;
    Args A;
    A.P = e->P; A.B = e->B; A.method = e->method;
    A.rho = e->inflation;
    A.y = e->y; A.ys = e->y_stride;
    A.obs = e->obs; A.obs_var = e->obs_var; A.active = e->active; A.eps = e->eps;
    A.status = e->status; A.stats = e->stats;
    for (int i = 0; i < e->n_arrays; i++) {
        const hbvx_enkf_array &a = e->a[i];
        A.in = a.in; A.out = a.out; A.n = a.n; A.M = a.M;
        A.lo = (double)a.lo;
        A.lead = i == 0;
        for (int64_t e0 = 0; e0 < a.n; e0 += piece) {
            A.e0 = e0;
            A.count = a.n - e0 < piece ? a.n - e0 : piece;
            const dim3 grid((unsigned)((A.count + THREADS - 1) / THREADS));
            if (A.rho != 1.0) hipLaunchKernelGGL(k_enkf<true>, grid, dim3(THREADS), 0, st, A);
            else hipLaunchKernelGGL(k_enkf<false>, grid, dim3(THREADS), 0, st, A);
            hipError_t err = hipGetLastError();
            if (err != hipSuccess) return hip_fail(err, "hbvx_enkf_update launch");
        }
    }
    return HBVX_OK;
}
