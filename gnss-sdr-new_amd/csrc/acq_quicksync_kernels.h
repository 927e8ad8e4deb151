// Device side of the QuickSync acquisition (pcps_quicksync_acquisition_cc.cc:265-472): what
// the plain search does not have.  An item is L = p spc samples; a Doppler row is the
// correlation, on Nf = spc / p points, of the folded wiped-off item with the folded code.
//
//   acq_forward_fold_kernel     X_{b,d} = FFT(fold(x_b .* w_d)): acq_forward_kernel with the
//   acq_forward_fold_pk_kernel  fold as its load functor (LDS plans and the packed plan)
//   acq_quick_candidate_kernel  |acc_i|^2 of the p delays the folded winner stands for
//
// The kernels that are no templates (code fold, record merge) are in acq_quicksync.hip.
#pragma once
#include "acq_kernels.h"

namespace
{

// ---------------------------------------------------------------- K_forward, folding
// sum_{k < segments} x[first + k n] w[k n]: four segments' loads in flight per round.
template <int IT>
__device__ __forceinline__ float2 fold_load(const void* __restrict__ iq, size_t first, const float2* __restrict__ w,
    uint32_t n, uint32_t segments)
{
    float2 acc = make_float2(0.f, 0.f);
    uint32_t k = 0;
    for (; k + 4 <= segments; k += 4)
        {
            float2 x[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                {
                    const size_t j = (size_t)(k + u) * n;
                    x[u] = load_item<IT>(iq, first + j);
                    c[u] = w[j];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                {
                    const float2 v = gsdr::fft::cmul(x[u], c[u]);
                    acc.x += v.x;
                    acc.y += v.y;
                }
        }
    for (; k < segments; ++k)
        {
            const size_t j = (size_t)k * n;
            const float2 v = gsdr::fft::cmul(load_item<IT>(iq, first + j), w[j]);
            acc.x += v.x;
            acc.y += v.y;
        }
    return acc;
}

// load(i) = sum_{k < segments} x[base + i + k Nf] w_d[i + k Nf], segments = p^2 (:329, :336-343):
// every k reads consecutive i across the lanes.  w_d is a row of L = segments Nf samples;
// with the spectrum reuse (XMap) the stored rows are those of Doppler bins 0..q-1: the
// wipe-off of bin c + a q is w_c[n] exp(-j 2 pi a p n / Nf), and n = i + k Nf leaves
// exp(-j 2 pi a p i / Nf) whatever the segment, so the fold of bin c + a q is the fold of
// bin c shifted by a p bins of its spectrum, as in the plain search.
template <class PT, int IT>
__global__ void __launch_bounds__(PT::NT) acq_forward_fold_kernel(const void* __restrict__ iq, uint64_t item_stride,
    const float2* __restrict__ wipe, float2* __restrict__ X, const float2* __restrict__ tw, typename PT::PlanT plan,
    uint32_t segments, XMap xm)
{
    extern __shared__ float2 lds[];
    const uint32_t b = blockIdx.x, d = blockIdx.y;
    const uint32_t n = (uint32_t)plan.n;
    const size_t base = (size_t)b * item_stride;
    const float2* w = wipe + (size_t)d * segments * n;
    float2* out = X + xm.off(b, d);
    const int ext = (int)(xm.stride - n);  // bins repeated after N - 1 (XMap)
    auto load = [&](int i) -> float2 {
        if (i >= (int)n) return make_float2(0.f, 0.f);
        return fold_load<IT>(iq, base + (uint32_t)i, w + i, n, segments);
    };
    auto store = [&](int i, float2 v) {
        out[i] = v;
        if (i < ext) out[n + i] = v;
    };
    PT::run(plan, lds, tw, load, store);
}

// The same on the packed plan (the X layout of the packed correlate variants).
template <class MP, int IT>
__global__ void __launch_bounds__(MP::NT) acq_forward_fold_pk_kernel(const void* __restrict__ iq, uint64_t item_stride,
    const float2* __restrict__ wipe, float2* __restrict__ X, const float2* __restrict__ tw, uint32_t segments, XMap xm)
{
    using gsdr::pk::c2;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    const uint32_t b = blockIdx.x, d = blockIdx.y;
    constexpr uint32_t N = MP::N;
    const size_t base = (size_t)b * item_stride;
    const float2* w = wipe + (size_t)d * segments * N;
    c2* out = reinterpret_cast<c2*>(X) + xm.off(b, d);
    const int ext = (int)(xm.stride - N);  // bins repeated after N - 1 (XMap)
    auto load = [&](int, int, int i) -> c2 {
        if (i >= (int)N) return c2{0.f, 0.f};
        return gsdr::pk::from(fold_load<IT>(iq, base + (uint32_t)i, w + i, N, segments));
    };
    auto store = [&](int i, c2 v, int) {
        out[i] = v;
        if (i < ext) out[N + i] = v;
    };
    MP::run(lds, tw, load, store, [] {});
}

// ---------------------------------------------------------------- K_candidate
// The check of the p delays (:383-412) of the winner (row d, folded phase t) that the reduce
// pass left in res[b nprn + slot]: acc_i = sum_{j < spc} x[t + i Nf + j] w_d[t + i Nf + j] code[j],
// the code not conjugated (volk_32fc_x2_multiply_32fc, :403), and cand[(b nprn + slot) p + i] =
// |acc_i|^2.  The last read is sample (Nf - 1) + (p - 1) Nf + spc - 1 = 2 spc - 2 < L for p >= 2.
// w_d is the row's own wipe-off: the stored row c = d mod q times the shift's phasor
// W_Nf^{a p (n mod Nf)}, a = d / q, from the handle's twiddle table (XMap; p = 0: the row itself).
// blockIdx.x = b nprn + slot, blockIdx.y = i (gridDim.y = p): one workgroup per candidate.
constexpr int kQuickCandLanes = 1024;

template <int IT>
__global__ void __launch_bounds__(kQuickCandLanes) acq_quick_candidate_kernel(const void* __restrict__ iq,
    uint64_t item_stride, const float2* __restrict__ wipe, const float2* __restrict__ tw,
    const float2* __restrict__ codes, const gsdr_acq_result* __restrict__ res, float* __restrict__ cand, uint32_t nprn,
    uint32_t D, uint32_t p, uint32_t spc, uint32_t nf, XMap xm)
{
    constexpr int NW = kQuickCandLanes / 64;
    __shared__ float2 s_acc[NW];
    const uint32_t bp = blockIdx.x, i = blockIdx.y;
    const uint32_t b = bp / nprn, slot = bp - b * nprn;
    // the device record's winner, kept inside the grid whatever it holds
    const uint32_t d = min(res[bp].doppler_index, D - 1);
    const uint32_t t = min(res[bp].code_phase, nf - 1);
    const uint32_t a = d / xm.q, c = d - a * xm.q, shift = a * xm.p;
    const size_t base = (size_t)b * item_stride;
    const float2* w = wipe + (size_t)c * p * spc;
    const float2* code = codes + (size_t)slot * spc;
    const uint32_t delay = t + i * nf;
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll 2
    for (uint32_t j = threadIdx.x; j < spc; j += kQuickCandLanes)
        {
            const uint32_t n = delay + j;
            float2 wv = w[n];
            if (shift) wv = gsdr::fft::cmul(wv, tw[(shift * (n % nf)) % nf]);
            const float2 y = gsdr::fft::cmul(gsdr::fft::cmul(load_item<IT>(iq, base + n), wv), code[j]);
            acc.x += y.x;
            acc.y += y.y;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            acc.x += __shfl_xor(acc.x, off);
            acc.y += __shfl_xor(acc.y, off);
        }
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        {
            float2 tot = make_float2(0.f, 0.f);
#pragma unroll
            for (int wv = 0; wv < NW; ++wv)
                {
                    tot.x += s_acc[wv].x;
                    tot.y += s_acc[wv].y;
                }
            cand[(size_t)bp * p + i] = tot.x * tot.x + tot.y * tot.y;
        }
}

}  // namespace
