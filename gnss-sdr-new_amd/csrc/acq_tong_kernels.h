// Tong acquisition (pcps_tong_acquisition_cc): the grid kernel template over the LDS plan
// types.  The launch code, the counter kernel and the C ABI are in acq_tong.hip.
#pragma once
#include "acq_kernels.h"

namespace
{

using gsdr_acq_impl::TongSlot;

// ---------------------------------------------------------------- K_tong_grid
// The accumulated grid of a call's items (:312-322).  Row (d, p) after item k depends only on
// row (d, p) after item k - 1, so one workgroup owns the row for the whole call: blockIdx.x =
// d P + p (consecutive workgroups share the spectra X_{k,d}).  For k ascending it transforms
// conj(X_{k,d}) C_p as acq_correlate_kernel does, and in the store functor forms
// m = |v|^2 s_k (the multiply, :312-314) and acc = acc + m (the add, :317), each rounded once,
// in the reference's order.  Where the running row waits between items:
//   ROW_LDS   in LDS behind the transform's buffer and the statistics scratch (4 N bytes
//             more): copied in from the HBM row before the first item -- zeros instead where
//             the slot's sequence starts with this call (TongSlot::dwell_count == 0: the
//             reference zeroes the grid at restart, :203-209, :244-250), the HBM row is then
//             not read at all -- and copied out after the last, both in lane-consecutive
//             order.  The store functor is lrow[i] += m and nothing else;
//   otherwise in the workgroup's own row of the HBM grid, which no other workgroup touches;
//             the first item of a starting sequence skips the read.
// The lane that stores output i of one item stores output i of every item (the plan's index
// map depends on the lane alone), so between the items element i is private to a lane; the
// copies in and out are fenced by barriers.  After every item the row's (maximum, first index)
// goes to stats[(k P + p) D + d]: the lane visits its outputs in no fixed index order, so
// stat_better keeps the smaller index among equals.
//
// A slot whose sequence has ended before the call takes no part: its items are all past the
// end, and the workgroup leaves at once.  Items computed after a sequence ends inside the call
// are speculation that acq_tong_update_kernel ignores; the grid they leave is discarded by the
// reset that must precede the slot's next sequence.
template <class PT, bool ROW_LDS>
__global__ void __launch_bounds__(PT::NT) acq_tong_grid_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, const float2* __restrict__ tw,
    typename PT::PlanT plan, float* __restrict__ grid, const float* __restrict__ scale,
    const TongSlot* __restrict__ slots, uint32_t D, uint32_t P, uint32_t nitems, XMap xm)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    float* lrow = reinterpret_cast<float*>(scratch + 16);
    const uint32_t N = plan.n;
    const uint32_t d = blockIdx.x / P, p = blockIdx.x - d * P;
    const TongSlot sl = slots[p];
    if (sl.state != GSDR_TONG_RUNNING) return;
    const bool fresh = sl.dwell_count == 0;
    float* row = grid + ((size_t)p * D + d) * N;
    const float2* c = code_fft + (size_t)p * N;
    if (ROW_LDS)
        {
            for (uint32_t i = threadIdx.x; i < N; i += PT::NT) lrow[i] = fresh ? 0.0f : row[i];
            __syncthreads();
        }
#pragma unroll 1
    for (uint32_t k = 0; k < nitems; ++k)
        {
            const float2* x = X + xm.off(k, d);
            const float s = scale[k];
            const bool from_zero = !ROW_LDS && fresh && k == 0;
            // the code row and the twiddles are the same for every item: left visible, the
            // compiler hoists their loads out of the item loop and keeps them all live (2-3 times
            // the registers of acq_dwell_grid_kernel, scratch on the 1024-lane plan)
            const float2* ck = c;
            const float2* twk = tw;
            asm volatile("" : "+v"(ck), "+v"(twk));
            float best = -1.0f, sum = 0.0f;
            uint32_t bidx = 0xffffffffu;
            auto load = [&](int i) -> float2 {
                float2 a = x[i], q = ck[i];
                return make_float2(a.x * q.x + a.y * q.y, a.x * q.y - a.y * q.x);
            };
            auto store = [&](int i, float2 v) {
                const float m = gsdr::mul_rn(v.x * v.x + v.y * v.y, s);
                float acc;
                if (ROW_LDS)
                    {
                        acc = gsdr::add_rn(lrow[i], m);
                        lrow[i] = acc;
                    }
                else
                    {
                        float prev = 0.0f;
                        if (!from_zero) prev = row[i];
                        acc = gsdr::add_rn(prev, m);
                        row[i] = acc;
                    }
                if (stat_better(acc, (uint32_t)i, best, bidx))
                    {
                        best = acc;
                        bidx = (uint32_t)i;
                    }
            };
            PT::run(plan, lds, twk, load, store);
            block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
            if (threadIdx.x == 0) stats[((size_t)k * P + p) * D + d] = RowStat{best, bidx, 0.0f, 0};
            // the scratch and the transform's buffer are free for the next item, and the row is
            // whole for the copy out
            __syncthreads();
        }
    if (ROW_LDS)
        for (uint32_t i = threadIdx.x; i < N; i += PT::NT) row[i] = lrow[i];
}

}  // namespace
