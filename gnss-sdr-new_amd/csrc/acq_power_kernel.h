// d_input_power of the blocks that measure it on the items themselves: the paired-code
// blocks over fft_size samples (acq_pair.hip) and QuickSync over an item of p
// samples_per_code (acq_quicksync.hip).
#pragma once
#include "acq_kernels.h"

namespace
{

// volk_32fc_magnitude_squared_32f, volk_32f_accumulator_s32f, / n (pcps_cccwsr_acquisition_cc.cc:250-252,
// pcps_quicksync_acquisition_cc.cc:310-312) of block b's n items: a float partial sum per lane,
// reduced across the workgroup.
constexpr int kPairPowerLanes = 1024;  // one workgroup per block: many loads in flight per lane round

template <int IT>
__global__ void __launch_bounds__(kPairPowerLanes) acq_pair_power_kernel(const void* __restrict__ iq, uint64_t block_stride,
    uint32_t n, float* __restrict__ power)
{
    constexpr int NW = kPairPowerLanes / 64;
    __shared__ float s_sum[NW];
    const uint32_t b = blockIdx.x;
    const size_t base = (size_t)b * block_stride;
    float acc = 0.0f;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < n; i += kPairPowerLanes)
        {
            const float2 x = load_item<IT>(iq, base + i);
            acc = __builtin_fmaf(x.x, x.x, __builtin_fmaf(x.y, x.y, acc));
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        {
            float tot = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += s_sum[w];
            power[b] = tot / (float)n;
        }
}

}  // namespace
