// Split register four-step correlate (acq_correlate_split_kernel,
// acq_split_kernels.h) for the FFT sizes of configs C4 / C5 beyond the LDS engine:
// plan choice, launch and one-time setup, selected by gsdr_acq::split.
#include "acq_handle.h"
#include "acq_split_kernels.h"

namespace gsdr_acq_impl
{
namespace
{

// Inner M-point register four-step plans (RegFourStep<R, NT, H, WPE, pads, row radices>):
//   25000 = 25 x (10 x 10 x 10): 512 lanes, two columns per lane (50 complex in
//           VGPRs), 5 rows of 1000 per LDS round (40 KB)
//   32000 = 32 x (10 x 10 x 10) with wave-local rows (H = 0): 1024 lanes, one column
//           per lane (32 complex), each LDS round holds one row per wave and every
//           wave transforms its row without workgroup barriers; rounds 16 + 16 (128 KB)
using Reg25k = RegFourStep<25, 512, 5, 1, NoPads<1000>, 10, 10, 10>;
using Wl32k = RegFourStep<32, 1024, 0, 1, NoPads<1000>, 10, 10, 10>;
// 25000 = 25 x (10 x 10 x 10) on 1024 lanes, one column per lane, 10 rows per LDS
// round: the plan of the two-sub-transform workgroups (QPW 2) of 100000 = 4 x 25000
using Reg25kW = RegFourStep<25, 1024, 10, 1, NoPads<1000>, 10, 10, 10>;

// A split: N = ROUT x RP::N, QPW sub-transforms or PPW PRNs per workgroup.
template <int ROUT_, class RP_, int QPW_ = 1, int PPW_ = 1>
struct Split
{
    static constexpr int ROUT = ROUT_, QPW = QPW_, PPW = PPW_;
    using RP = RP_;
};

// The split ids: f(Split, std::bool_constant<half>) for the handle's.
//   1: 25000 = 1 x 25000 (C5 GPS L1 / BeiDou B1I at 25 Msps, 1 ms)
//   25: the same, two PRNs per 1024-lane workgroup (AcqEnv::ppw 2)
//   4: 100000 = 4 x 25000 (C5 Galileo E1 at 25 Msps, 4 ms), one sub-transform per workgroup
//   24: the same, two sub-transforms (q, q + 2) per 1024-lane workgroup (the default)
//   12: 32000 = 1 x Wl32k (Galileo E1 at 8 Msps, 4 ms)
//   13: 64000 = 2 x Wl32k (C4: Galileo E1 at 8 Msps with bit transition)
// Measured and removed: round 4's 100000 = 2 x 50000 (25 x 2000 register
// four-step, 164 B/lane of spills, -3.5 %), the outer DIF step as its own pass (-11 % /
// -29 %), mirror-pair loads of the Hermitian code spectra (within +-3 %); round 5's
// round 6's 25000 alternatives (profiles/r06j): 10-row LDS rounds on 512 lanes (capped at
// 128 VGPRs, -3-5 %) and one column per lane on 1024 lanes (-22 %); round 5's
// pruning of the alternatives that lost their A/Bs: 32000 / 64000 on 8-row LDS rounds
// (ids 2 / 3, -4 % / -10 %), the 16000-based splits (5 / 6), the wave-local 25000 /
// 100000 plans (11 / 14 / 17 / 18, -25 % / -20 % at 25000), 2 x / 4 x 16000 wave-local
// (15 / 16), the bank-model padded rows (19 / 20 and 7 / 8: conflicts halved, time
// unchanged, profiles/r05p).
template <class F>
int with_split(int id, bool half, F&& f)
{
    auto halves = [&](auto sp) { return half ? f(sp, std::true_type{}) : f(sp, std::false_type{}); };
    switch (id)
        {
        case 1: return halves(Split<1, Reg25k>{});
        case 25: return halves(Split<1, Reg25kW, 1, 2>{});
        case 4: return halves(Split<4, Reg25k>{});
        case 24: return halves(Split<4, Reg25kW, 2>{});
        case 12: return halves(Split<1, Wl32k>{});
        case 13: return halves(Split<2, Wl32k>{});
        default: gsdr::set_error("internal: bad split variant %d", id); return GSDR_E_STATE;
        }
}

// one plan per size (r04a: wave-local rows 12 / 13 for 32000 / 64000, +4 % / +10 %
// over 8-row LDS rounds; the 512-lane 25000 plan keeps its LDS rounds)
int split_for(const gsdr_acq* a)
{
    switch (a->N)
        {
        case 25000: return a->env.ppw == 2 ? 25 : 1;
        case 32000: return 12;
        case 64000: return 13;
        case 100000: return a->env.qpw == 2 ? 24 : 4;
        default: return 0;
        }
}

// PRN group of an XCD pass: the largest divisor of P whose code rows fit in ~2 MB
// (half an XCD's L2), so the rows of the group's codes stay resident while the X
// rows stream past
uint32_t prn_group(uint32_t P, uint32_t N)
{
    const size_t row = (size_t)N * sizeof(float2);
    // code bytes per group walked by every XCD at once: 2 MB (r04x: 1 MB within
    // noise, 4 MB -7 % at Galileo, 8 MB -10-12 %: the per-XCD L2 sets it; r06g2 with
    // warm clocks: 0.5 / 1 / 4 MB within noise, 8 MB -15 % at 25000)
    constexpr size_t cap = (size_t)2 << 20;
    uint32_t best = 1;
    for (uint32_t g = 1; g <= P; ++g)
        if (P % g == 0 && (size_t)g * row <= cap) best = g;
    return best;
}

// ARG = false: the grid pass (row maxima into d_stats); ARG = true: the selected
// rows' pass (keys into d_keys, |R|^2 rows into rowbuf for the peak ratio; the
// caller zeroes d_keys and runs acq_argmax_split_finish_kernel)
template <int ROUT, class RP, bool HALF, bool ARG = false, int QPW = 1, int PPW = 1>
int launch_one(gsdr_acq* a, const AcqView& v, uint32_t nblocks, hipStream_t s, const gsdr_acq_result* sel = nullptr,
    float* rowbuf = nullptr, float* psum = nullptr)
{
    static_assert(RP::N * ROUT > 0, "plan");
    if (RP::N * ROUT != (int)a->N)
        {
            gsdr::set_error("internal: split plan for N = %d, handle N = %u", RP::N * ROUT, a->N);
            return GSDR_E_STATE;
        }
    if (ROUT > 1 && !ARG)
        GSDR_HIP(hipMemsetAsync(a->d_stats, 0, (size_t)nblocks * v.nprn * v.D * sizeof(RowStat), s));
    constexpr uint32_t RQ = ROUT / QPW;  // workgroups per transform
    if (v.nprn % PPW != 0)
        {
            gsdr::set_error("internal: %d PRNs per workgroup with %u PRNs", PPW, v.nprn);
            return GSDR_E_STATE;
        }
    const uint32_t grid = ARG ? nblocks * v.nprn * RQ : nblocks * v.D * (v.nprn / PPW) * RQ;
    hipLaunchKernelGGL((acq_correlate_split_kernel<ROUT, RP, HALF, ARG, QPW, PPW>), dim3(grid), dim3(RP::NT),
        (split_lds_bytes<ROUT, RP, PPW>()), s, a->d_X, v.code_fft, a->d_stats, a->d_tw, v.D, v.nprn, nblocks,
        prn_group(v.nprn / PPW, a->N * PPW), v.xm, sel, a->d_keys, rowbuf, psum);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

// The grid pass (with PPW also its one-PRN form) and the selected rows' pass.
template <int ROUT, class RP, bool HALF, int QPW = 1, int PPW = 1>
int attrs_one()
{
    int rc = set_max_lds((const void*)acq_correlate_split_kernel<ROUT, RP, HALF, false, QPW, PPW>,
        split_lds_bytes<ROUT, RP, PPW>());
    rc |= set_max_lds((const void*)acq_correlate_split_kernel<ROUT, RP, HALF, true, QPW>, split_lds_bytes<ROUT, RP>());
    if constexpr (PPW > 1) rc |= attrs_one<ROUT, RP, HALF, QPW>();
    return rc;
}

}  // namespace

int launch_split_argmax(gsdr_acq* a, const AcqView& v, uint32_t nblocks, gsdr_acq_result* res, hipStream_t s)
{
    const bool half = a->eff != a->N;
    const AcqParams ap = params_of(a, v);
    GSDR_HIP(hipMemsetAsync(a->d_keys, 0, (size_t)nblocks * v.nprn * sizeof(unsigned long long), s));
    float* rowbuf = ap.cfar ? nullptr : a->d_rowbuf;
    // CFAR (not in step two, whose input power is the first step's): the Parseval
    // shares of the opposite row come from the split pass itself
    float* psum = (ap.cfar && !ap.step_two && !half) ? a->d_psum : nullptr;
    uint32_t rout = 1;
    // the selected rows' pass: one PRN per workgroup on the handle's split plan
    int rc = with_split(a->split, half, [&](auto sp, auto h) {
        using S = decltype(sp);
        rout = S::ROUT;
        return launch_one<S::ROUT, typename S::RP, decltype(h)::value, true, S::QPW>(a, v, nblocks, s, res, rowbuf, psum);
    });
    if (rc != GSDR_OK) return rc;
    hipLaunchKernelGGL((acq_argmax_split_finish_kernel<1024>), dim3(nblocks * v.nprn), dim3(1024), 0, s, a->d_X,
        v.code_fft, res, a->d_keys, rowbuf, psum, rout, ap);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

int launch_split(gsdr_acq* a, const AcqView& v, uint32_t nblocks, hipStream_t s)
{
    return with_split(a->split, a->eff != a->N, [&](auto sp, auto h) {
        using S = decltype(sp);
        constexpr bool HALF = decltype(h)::value;
        // an odd active PRN count: one PRN per workgroup on the same plan
        if (S::PPW > 1 && v.nprn % S::PPW != 0) return launch_one<S::ROUT, typename S::RP, HALF, false, S::QPW>(a, v, nblocks, s);
        return launch_one<S::ROUT, typename S::RP, HALF, false, S::QPW, S::PPW>(a, v, nblocks, s);
    });
}

// Select the split correlate for a single-dwell four-step handle (K = 1, with or
// without bit transition): 25000 / 32000 (ROUT = 1), 64000 = 2 x 32000 (C4 bit
// transition: 52 -> 61 Msps, profiles/r03q) and 100000 = 4 x 25000.  The last was
// slower than the packed four-step (87 vs 100 Msps: every sub-transform re-reads the
// whole X and code rows) until the forward-spectrum reuse (XMap) left one X row per
// block in L2: 116 vs 107 Msps (profiles/r04h).
int setup_split(gsdr_acq* a)
{
    a->split = 0;
    // non-coherent dwells run the accumulating general path
    const int id = (a->K == 1 && a->env.split) ? split_for(a) : 0;
    if (!id) return GSDR_OK;
    auto attrs = [](auto sp, auto h) {
        using S = decltype(sp);
        return attrs_one<S::ROUT, typename S::RP, decltype(h)::value, S::QPW, S::PPW>();
    };
    if ((with_split(id, true, attrs) | with_split(id, false, attrs)) != GSDR_OK) return GSDR_E_DEVICE;
    a->split = id;
    return GSDR_OK;
}

}  // namespace gsdr_acq_impl
