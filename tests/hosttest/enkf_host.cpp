// enkf_host.cpp -- the body of hbvx_enkf_update (hydrodl2_amd/csrc/hbv_enkf.h) compiled for the host: a plain loop over the
// elements of one array, as the kernel's threads take them (tests/test_enkf_host.py, tests/test_enkf_gpu.py).
#include <cstdint>

#include "../../hydrodl2_amd/csrc/hbv_enkf.h"

using namespace hbvx_enkfk;

// The arguments are those of hbvx_enkf (include/hbvx_enkf.h) for ONE array; lead: this array stores status and stats, and
// status is cleared first, as the launcher does.  form 0: the instance the call's rho selects; form 1: the instance
// WITHOUT inflation whatever rho is (what rho == 1 must have the bits of).
extern "C" void enkf_host(int P, int B, int method, double rho, const float *y, int64_t ys, const float *obs,
                          const float *obs_var, const uint8_t *active, const float *eps, int *status, double *stats,
                          const float *in, float *out, int64_t n, int M, float lo, int lead, int form)
{
    Args A;
    A.P = P; A.B = B; A.method = method;
    A.rho = rho;
    A.y = y; A.ys = ys;
    A.obs = obs; A.obs_var = obs_var; A.active = active; A.eps = eps;
    A.status = status; A.stats = stats;
    A.in = in; A.out = out; A.n = n; A.M = M;
    A.lo = (double)lo;
    A.e0 = 0; A.count = n;
    A.lead = lead;
    if (lead && status)
        for (int b = 0; b < B; b++) status[b] = 0;
    for (int64_t e = 0; e < n; e++) {
        if (form == 1) element<false>(A, e);
        else element_of(A, e);
    }
}
