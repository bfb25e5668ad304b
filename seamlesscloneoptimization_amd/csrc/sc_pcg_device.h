// sc_pcg_device.h -- what the kernels of the two conjugate-gradient families share (sc_weighted.hip, sc_wls.hip): the workgroup's size, its
// sum in one fixed order, and the segment of a plane that one workgroup of an element-wise launch owns (sc_common.h, WeightedGeo).
#pragma once
#include "sc_common.h"
#include "sc_wave.h"
#include <algorithm>

namespace sc {

constexpr int WL = 256;      // lanes per workgroup

// the workgroup's sum (valid in every lane after the barrier); ws: 4 doubles of LDS of this call's own
__device__ __forceinline__ double block_sum(double v, double *ws)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// the float4 groups [g0, g1) of a plane of n floats that segment `part` owns
__device__ __forceinline__ void segment(const WeightedGeo &wg, int part, int &g0, int &g1)
{
    const int per = (wg.egroups + wg.eparts - 1) / wg.eparts;
    g0 = part * per;
    g1 = min(g0 + per, wg.egroups);
}

// a * b rounded to float32 on its own: never one half of a fused multiply-add, whatever the translation unit's contraction setting
// (the product is opaque to the optimiser, as in screened_rhs)
__device__ __forceinline__ float rounded_product(float a, float b)
{
    float t = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));
#endif
    return t;
}

} // namespace sc
