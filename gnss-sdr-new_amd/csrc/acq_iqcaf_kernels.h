// E5a non-coherent IQ acquisition with CAF filter
// (galileo_e5a_noncoherent_iq_acquisition_caf_cc): the grid kernel template over every plan
// type.  The replica, finish and launch code and the C ABI are in acq_iqcaf.hip.
#pragma once
#include "acq_kernels.h"

namespace
{

// What thread 0 leaves for the workgroup between the slots' transforms and the sum pass.
struct IqCafStash
{
    float peak[4];
    uint32_t idx[4];
    uint32_t choice_i, choice_q;
    uint32_t pad[6];
};
static_assert(sizeof(IqCafStash) == 64, "kIqCafStash (acq_handle.h)");

// ---------------------------------------------------------------- K_iqcaf_grid
// One workgroup per (Doppler row d, satellite, item): blockIdx.x = d nsat + sat (consecutive
// workgroups share the spectrum X_{k,d}), blockIdx.y = item k.  The satellite's code slots are
// sat nslots + s in the order I-A, [I-B], [Q-A], [Q-B] (B forms with coherent_ms > 1, Q forms
// with both components).  For s ascending -- a loop that is not unrolled, so the transform is
// inlined once -- it transforms conj(X_{k,d}) C_s as acq_correlate_kernel does, the store functor
// writing |z|^2 to row buffer s and keeping the lane's (maximum, first index); thread 0 stashes
// the row's statistic.  Then thread 0 makes the reference's selection (:415-546) in scalar code:
// the quotients peak / (fn fn), fn = float(N) float(N), in float; A where its quotient is '>='
// B's; and magt_QB is the I-B row read at Q-B's index (:445), as the reference has it.  After a
// barrier every lane adds the two chosen rows cell by cell, one rounded add each, and the
// workgroup reduces the sum's (maximum, first index); with one component the row's value is the
// chosen I row's own statistic.
//
// Where the rows wait: ROWS_LDS in LDS behind the transform's buffer, the statistics scratch and
// the stash; otherwise in the workgroup's own region of `hrows`, (k nsat + sat) D + d, of
// nslots N floats, which no other workgroup touches.  A cell is written by one lane during the
// transform and read by another in the sum pass (and by thread 0 for :445): the barrier at the
// end of every slot's round orders them, the region staying within the workgroup's CU.
template <class PT, bool ROWS_LDS>
__global__ void __launch_bounds__(PT::NT) acq_iqcaf_grid_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_iq_caf_row* __restrict__ rec, const float2* __restrict__ tw,
    typename PT::PlanT plan, float* hrows, uint32_t D, uint32_t nsat, uint32_t nslots, uint32_t both, XMap xm)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    IqCafStash* stash = reinterpret_cast<IqCafStash*>(scratch + 16);
    const uint32_t N = plan.n;
    const uint32_t d = blockIdx.x / nsat, sat = blockIdx.x - d * nsat, k = blockIdx.y;
    const size_t region = ((size_t)k * nsat + sat) * D + d;
    float* rows = ROWS_LDS ? reinterpret_cast<float*>(stash + 1) : hrows + region * nslots * N;
    const float2* x = X + xm.off(k, d);
    const float2* c0 = code_fft + (size_t)sat * nslots * N;
#pragma unroll 1
    for (uint32_t s = 0; s < nslots; ++s)
        {
            const float2* c = c0 + (size_t)s * N;
            float* row = rows + (size_t)s * N;
            float best = -1.0f, sum = 0.0f;
            uint32_t bidx = 0xffffffffu;
            auto load = [&](int i) -> float2 {
                float2 a = x[i], q = c[i];
                return make_float2(a.x * q.x + a.y * q.y, a.x * q.y - a.y * q.x);
            };
            auto store = [&](int i, float2 v) {
                const float m = v.x * v.x + v.y * v.y;
                row[i] = m;
                if (stat_better(m, (uint32_t)i, best, bidx))
                    {
                        best = m;
                        bidx = (uint32_t)i;
                    }
            };
            PT::run(plan, lds, tw, load, store);
            block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
            if (threadIdx.x == 0)
                {
                    stash->peak[s] = best;
                    stash->idx[s] = bidx;
                }
            // the scratch and the transform's buffer are free for the next slot, and the row is whole
            __syncthreads();
        }
    const bool has_b = (both ? nslots == 4 : nslots == 2);
    const uint32_t qa = has_b ? 2u : 1u;  // slot of Q-A
    if (threadIdx.x == 0)
        {
            const float fn = gsdr::mul_rn((float)N, (float)N);
            const float fn2 = gsdr::mul_rn(fn, fn);
            uint32_t ci = 0, cq = 0;
            if (has_b)
                {
                    const float magt_ia = stash->peak[0] / fn2, magt_ib = stash->peak[1] / fn2;
                    ci = magt_ia >= magt_ib ? 0u : 1u;
                    if (both)
                        {
                            const float magt_qa = stash->peak[2] / fn2;
                            // :445: d_magnitudeIB[indext_QB] (a row of NaNs leaves no index: cell 0)
                            const uint32_t iqb = stash->idx[3] < N ? stash->idx[3] : 0u;
                            const float magt_qb = rows[(size_t)N + iqb] / fn2;
                            cq = magt_qa >= magt_qb ? 0u : 1u;
                        }
                }
            stash->choice_i = ci;
            stash->choice_q = cq;
        }
    __syncthreads();
    const uint32_t ci = stash->choice_i, cq = stash->choice_q;
    float best, sum = 0.0f;
    uint32_t bidx;
    if (both)
        {
            const float* ri = rows + (size_t)ci * N;
            const float* rq = rows + (size_t)(qa + cq) * N;
            best = -1.0f;
            bidx = 0xffffffffu;
            for (uint32_t i = threadIdx.x; i < N; i += PT::NT)
                {
                    const float m = gsdr::add_rn(ri[i], rq[i]);
                    // i ascends within the lane: '>' keeps its first maximum
                    if (m > best)
                        {
                            best = m;
                            bidx = i;
                        }
                }
            block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
        }
    else
        {
            best = stash->peak[ci];
            bidx = stash->idx[ci];
        }
    if (threadIdx.x == 0)
        {
            gsdr_acq_iq_caf_row r;
            r.choice_i = ci;
            r.choice_q = cq;
            r.peak_i = stash->peak[ci];
            r.peak_q = both ? stash->peak[qa + cq] : 0.0f;
            r.sum_peak = best;
            r.sum_index = bidx;
            rec[region] = r;
        }
}

}  // namespace
