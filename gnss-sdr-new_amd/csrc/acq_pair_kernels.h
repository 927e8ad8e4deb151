// Device side of the paired-code acquisition (pcps_cccwsr_acquisition_cc.cc:211-436,
// galileo_pcps_8ms_acquisition_cc.cc): what the plain search does not have.  Every
// satellite is searched with two replicas; the grid value of a Doppler row is the larger
// of the two members' row maxima.  The two correlations run on the engine's own forward
// and correlate kernels over two code slots per satellite (pair q: slots 2 q, 2 q + 1).
//
//   acq_pair_replica_kernel  the two staged code rows of each pair from the caller's
//                            two arguments (as they are, or first -+ j second)
//   acq_pair_power_kernel    d_input_power = sum |x|^2 / fft_size of each block (acq_power_kernel.h)
//   acq_pair_merge_kernel    the pair's record from its two slots' records
#pragma once
#include "acq_kernels.h"
#include "acq_power_kernel.h"

namespace
{

// Rows 2 q and 2 q + 1 of stage (n complex each) from rows q of first and second.
// GSDR_ACQ_PAIR_SUM_DIFF_J: first - j second and first + j second.  CCCWSR's
// d_correlation_plus = data + j pilot (:301-308) is, the correlation being conjugate-linear
// in the replica, the correlation with the one replica data - j pilot, and
// d_correlation_minus the one with data + j pilot.
__global__ void __launch_bounds__(256) acq_pair_replica_kernel(const float2* __restrict__ first,
    const float2* __restrict__ second, float2* __restrict__ stage, uint32_t n, int kind)
{
    const uint32_t q = blockIdx.x;
    const float2* f = first + (size_t)q * n;
    const float2* s = second + (size_t)q * n;
    float2* m0 = stage + (size_t)(2 * q) * n;
    float2* m1 = m0 + n;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        {
            const float2 a = f[i], b = s[i];
            if (kind == GSDR_ACQ_PAIR_SUM_DIFF_J)
                {
                    // -j b = (b.y, -b.x), +j b = (-b.y, b.x)
                    m0[i] = make_float2(a.x + b.y, a.y - b.x);
                    m1[i] = make_float2(a.x - b.y, a.y + b.x);
                }
            else
                {
                    m0[i] = a;
                    m1[i] = b;
                }
        }
}

// One lane per (block b, pair q).  Each slot's record holds its grid maximum, the first
// Doppler row holding it (strict '>' over rows) and the first index in that row, so the
// reference's scan -- per row the larger member, '>=' keeping the first (:322-331), then
// 'd_mag < magt' over rows (:334) -- finds: the larger peak; on equal peaks the smaller
// row; on equal rows member 0.  The normalisation divides by (float(N) float(N))^2 in
// float (:247, :316, :320): monotone, so applied after the comparison of the raw peaks
// it leaves the winner the reference's unless two different raw peaks round to one
// quotient, where the reference takes the earlier cell and this the larger raw value.
__global__ void __launch_bounds__(64) acq_pair_merge_kernel(const gsdr_acq_result* __restrict__ slots,
    const float* __restrict__ power, gsdr_acq_pair_result* __restrict__ out, uint32_t npairs, uint32_t n_records,
    float fft_size, uint32_t samples_per_code)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_records) return;
    const uint32_t b = i / npairs;
    const gsdr_acq_result r0 = slots[2 * (size_t)i], r1 = slots[2 * (size_t)i + 1];
    const bool second = r1.peak > r0.peak || (r1.peak == r0.peak && r1.doppler_index < r0.doppler_index);
    const gsdr_acq_result w = second ? r1 : r0;
    const float norm = fft_size * fft_size;
    gsdr_acq_pair_result r;
    r.prn = w.prn;
    r.doppler_index = w.doppler_index;
    r.code_phase = w.code_phase;
    r.member = second ? 1u : 0u;
    r.doppler_hz = w.doppler_hz;
    r.pad = 0;
    r.mag = w.peak / (norm * norm);
    r.input_power = power[b];
    r.test_statistic = r.mag / r.input_power;
    r.pad2 = 0.0f;
    r.acq_delay_samples = (double)(samples_per_code ? w.code_phase % samples_per_code : w.code_phase);
    r.samplestamp = w.samplestamp;
    out[i] = r;
}

}  // namespace
