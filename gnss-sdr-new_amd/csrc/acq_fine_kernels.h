// Device side of the fine-Doppler estimate (pcps_acquisition_fine_doppler_cc.cc:346-419,
// estimate_Doppler): the kernel template over the FFT plan type and the finish kernel.
//
// The reference wipes the code off 10 ms of signal (L = 10 N samples), pads to
// M = 8 L points, takes one M-point FFT and the first maximum of |X|^2.  The padded
// transform is a pruned-input one:
//   X[8 q + r] = sum_n ( y[n] e^{-2 pi i n r / M} ) e^{-2 pi i n q / L},  r < 8, q < L,
// eight L-point transforms of y times a phase ramp.  Residue r owns the outputs
// 8 q + r and runs as a workgroup of its own; the M-point spectrum is never stored.
#pragma once
#include "acq_kernels.h"

namespace
{

// e^{-2 pi i m / (8 L)} for 0 <= m < 8 L, the phase reduced in integers: the octant
// oct = floor(m / L) by three compare-subtracts, the remainder folded into
// [0, pi / 4] (a <= L is exact in fp32), one division and one sincospi there, the
// octant's symmetry applied to the pair.  The phase error is half an ulp of a / L at
// every m: no fp32 product n r and no accumulated phase.
__device__ __forceinline__ float2 fine_ramp(uint32_t m, uint32_t L)
{
    uint32_t oct = 0, rem = m;
    if (rem >= 4u * L)
        {
            rem -= 4u * L;
            oct = 4;
        }
    if (rem >= 2u * L)
        {
            rem -= 2u * L;
            oct += 2;
        }
    if (rem >= L)
        {
            rem -= L;
            oct += 1;
        }
    const uint32_t a = (oct & 1u) ? L - rem : rem;
    float s, c;
    sincospif(0.25f * ((float)a / (float)L), &s, &c);
    // theta = (pi / 4) (oct + rem / L): (cos theta, sin theta) from (c, s) of the folded angle
    const bool swap = ((oct + 1u) & 2u) != 0;       // octants 1, 2, 5, 6
    const bool negc = ((oct + 2u) & 4u) != 0;       // octants 2 .. 5: cos theta < 0
    const bool negs = (oct & 4u) != 0;              // octants 4 .. 7: sin theta < 0
    const float ct = swap ? s : c, st = swap ? c : s;
    return make_float2(negc ? -ct : ct, negs ? st : -st);  // e^{-i theta}
}

// blockIdx.x = request, blockIdx.y = residue r.  plan.n = L = 10 N.
//   load:  x[n] c'[n mod N] e^{-2 pi i n r / M}
//   store: |X[8 q + r]|^2 into the lane's (maximum, lowest index) key -- outputs may
//          arrive in any order -- and, for the spectrum dump, into spec[8 q + r]
// The workgroup's key goes into keys[request] by one 64-bit atomic maximum (zeroed by
// the host): |X|^2 bits above, ~index below, so the first maximum wins exact ties
// (volk_gnsssdr_32f_index_max_32u, KERN/32f_index_max_32u.h:446-467).
template <class PT, int IT>
__global__ void __launch_bounds__(PT::NT) acq_fine_kernel(const void* __restrict__ iq,
    const float2* __restrict__ codes, const gsdr_acq_fine_request* __restrict__ reqs,
    unsigned long long* __restrict__ keys, float* __restrict__ spec, const float2* __restrict__ tw,
    typename PT::PlanT plan, uint32_t N)
{
    constexpr int NW = PT::NT / 64;
    extern __shared__ float2 lds[];
    __shared__ unsigned long long s_key[NW];
    const uint32_t rq = blockIdx.x, r = blockIdx.y;
    const uint32_t L = (uint32_t)plan.n;
    const gsdr_acq_fine_request q = reqs[rq];
    const float2* c = codes + (size_t)q.code_slot * N;
    const uint32_t shift = q.code_phase;
    auto load = [&](int i) -> float2 {
        const uint32_t n = (uint32_t)i, j = n % N;
        // The reference aligns the replica with
        //   std::rotate(c, c + (N - shift), c + N - 1)     (:365-371)
        // whose range ends at N - 1, not N: only the first N - 1 samples rotate and
        // sample N - 1 stays in place (shift 0 and 1 both leave the row as it is).  Kept
        // as the reference has it: c'[j] = c[(j + N - shift) mod (N - 1)] for j < N - 1.
        uint32_t src = j;
        if (shift > 1u && j != N - 1u)
            {
                src = j + N - shift;  // < 2 N - 3
                if (src >= N - 1u) src -= N - 1u;
            }
        const float2 y = gsdr::fft::cmul(load_item<IT>(iq, n), c[src]);
        return gsdr::fft::cmul(y, fine_ramp(n * r, L));  // n r < 8 L = M <= 2^24
    };
    unsigned long long key = 0ull;
    auto store = [&](int o, float2 v) {
        const uint32_t k = 8u * (uint32_t)o + r;
        const float m = __builtin_fmaf(v.x, v.x, v.y * v.y);
        if (spec) spec[k] = m;
        const unsigned long long t = ((unsigned long long)__float_as_uint(m) << 32) | (0xffffffffu - k);
        key = t > key ? t : key;
    };
    PT::run(plan, lds, tw, load, store);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        {
            const unsigned long long t = __shfl_xor(key, o);
            key = t > key ? t : key;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        {
#pragma unroll
            for (int w = 1; w < NW; ++w) key = s_key[w] > key ? s_key[w] : key;
            __hip_atomic_fetch_max(&keys[rq], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

// One lane per request: the merged key's index and peak, fftFreqBins[index] as the
// reference forms it (:394-404) and the 1000 Hz test (:407-416).  The reference's
// operands are floats -- static_cast<float>(d_fs_in), static_cast<float>(k),
// static_cast<float>(fft_size_extended) -- and its literals 2.0 are doubles, so the
// product and the quotient are formed in double and rounded once by the store into
// the float vector; the comparison against Acq_doppler_hz (a double) is in double.
__global__ void acq_fine_finish_kernel(const unsigned long long* __restrict__ keys,
    const gsdr_acq_fine_request* __restrict__ reqs, gsdr_acq_fine_result* __restrict__ out, uint32_t nreq, float fs,
    uint32_t M)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nreq) return;
    const unsigned long long key = keys[i];
    uint32_t k = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    if (k >= M) k = 0;  // no output compared greater than the zeroed key
    const double half_m = (double)(float)M / 2.0;
    const float freq = k < M / 2u ? (float)((((double)fs / 2.0) * (double)(float)k) / half_m)
                                  : (float)((((double)(-fs) / 2.0) * (double)(float)(M - k)) / half_m);
    const double coarse = (double)reqs[i].coarse_doppler_hz;
    const bool ok = fabs((double)freq - coarse) < 1000.0;
    // field by field: the record's padding keeps the zeros the host put there
    gsdr_acq_fine_result* res = out + i;
    res->index = k;
    res->peak = __uint_as_float((uint32_t)(key >> 32));
    res->freq_hz = freq;
    res->doppler_hz = ok ? (double)freq : coarse;
    res->accepted = ok ? 1 : 0;
    res->pad = 0;
}

}  // namespace
