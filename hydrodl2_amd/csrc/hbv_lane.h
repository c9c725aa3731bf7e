// hbv_lane.h -- the lane mapping of every one-wave-per-64-lanes kernel: the recurrence kernels (k_fwd and k_bwd in
// hbvx.hip, k_tan in hbv_tan.h), the implicit scheme (hbv_adj_kernels.h) and the time-parallel adjoint
// (hbv_chunked.h), whose block index comes from its XCD-aware block map.  One wavefront lane per (basin, ensemble
// member), a basin's Mp members in adjacent lanes, so that the ensemble mean is a butterfly over lanes.  (The tiled
// families have their own NParamT / LaneT in hbv_tiled.h.)
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/hbvx.h"
#include "hbv_step.h"

namespace hbvx {

template <int MODEL, bool BETAET>
struct NParam {
    static constexpr int value = MODEL == MODEL_HBV10 ? (BETAET ? 13 : 12)
                               : MODEL == MODEL_HBV11P ? 14 : (MODEL == MODEL_HOURLY ? 19 : 16);
};

struct LaneId {
    int jm, b, j;   // padded member index, basin (clamped), member (clamped)
    bool active;    // lane maps to a real (basin, member)
    bool leader;    // first lane of a real basin
    int64_t n;      // b*M + j
};

// bx: the index of the wave's group of 64 >> lgMp basins
__device__ __forceinline__ LaneId lane_id(const hbvx_desc &d, int lgMp, int bx)
{
    LaneId L;
    const int lane = threadIdx.x & 63;
    const int Mp = 1 << lgMp;
    L.jm = lane & (Mp - 1);
    int b = bx * (64 >> lgMp) + (lane >> lgMp);
    L.active = (b < d.B) && (L.jm < d.M);
    L.leader = (b < d.B) && (L.jm == 0);
    L.b = b < d.B ? b : d.B - 1;
    L.j = L.jm < d.M ? L.jm : d.M - 1;
    L.n = (int64_t)L.b * d.M + L.j;
    return L;
}
__device__ __forceinline__ LaneId lane_id(const hbvx_desc &d, int lgMp) { return lane_id(d, lgMp, blockIdx.x); }

// sum over the Mp lanes of one basin (xor butterfly; every lane gets the sum)
__device__ __forceinline__ float ens_sum(float v, int lgMp)
{
    for (int s = 0; s < lgMp; s++) v += __shfl_xor(v, 1 << s, 64);
    return v;
}

} // namespace hbvx
