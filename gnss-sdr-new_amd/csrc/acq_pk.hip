// Packed-f32 forward / correlate / argmax variants, one per compile-time FFT size
// (N = 2000, 4000, 8000, 16000): launch and one-time setup, selected by
// gsdr_acq::corr_variant.
#include "acq_handle.h"
#include "acq_plans.h"
#include "acq_quicksync_kernels.h"
#include "acq_split_kernels.h"

namespace gsdr_acq_impl
{
namespace
{

// The variants whose correlate kernel is not acq_correlate_pk_kernel (their forward
// and argmax passes use the variant's PkPlan): 93 = N 16000 on the register
// four-step 16 x (10 x 10 x 10), 512 lanes, 8 rows per LDS round, each XCD's
// rows walked in groups of 16 PRNs.
using RegPlan93 = RegFourStep<16, 512, 8, 1 | (16 << 4), NoPads<1000>, 10, 10, 10>;
// 94: 93 with wave-local rows (two rounds of 8 rows, one per wave, no barriers
// inside a row transform)
using RegPlan94 = RegFourStep<16, 512, 0, 1 | (16 << 4), NoPads<1000>, 10, 10, 10>;

// A variant (default_pk_variant; GSDR_ACQ_CORR_VARIANT selects one for tests): id,
// plan, PRNs per workgroup, waves-per-EU hint, row statistic (1 max + sum with the
// argmax recomputed for the selected row, 2 max only with the CFAR row sum by
// Parseval -- see acq_correlate_pk_kernel), the code source (CodeSrc) and, for 93 / 94, the register four-step
// the correlate runs on instead (acq_correlate_reg_kernel, N = 16000, PRN-group-major
// XCD walk).  The alternatives measured in
// rounds 1-4 and removed: other radix orders, per-stage twiddle
// tables (-23 %) and LDS root copies (-2.5 %), padded layouts, late or dropped
// barriers, 5 waves per SIMD (with spills -19 %; without, the first-stage products
// in two halves, -2 %), 3 / 2 workgroups per CU (-8 % / -26 %), per-wave atomic row
// maxima (-2 %), multi-transform workgroups with both operand sets in VGPRs:
// variant 70 at 104 VGPRs runs 4 workgroups (16 waves) per CU, where the CU's
// issue, not latency, bounds it.  97 is 70's plan with X resident for 16 PRNs and
// the code rows staged through the drained FFT buffer (kCodeLds, 126 VGPRs under
// the 4-waves-per-SIMD hint, no scratch): +5 % on the C2 bench, bit-identical
// results; 70 stays as the tests' reference.  Groups of 4 and 8 PRNs (95, 96) gained
// +2 % and +3 % and were removed.  98 is 97 with the code rows copied from the
// handle's lane-order buffer (kCodeLane: each lane's 25 code values in its own output
// slots, so no barrier before the first stage's writes -- 5 per transform instead of
// 6 --, all 25 X values resident, code reads five ahead of their products, the idle
// wave skipping the first stage's reads and products; 128 VGPRs, no scratch,
// occupancy 4): +5 % over 97 on the C2 bench, bit-identical results; 97 stays as its
// A/B partner.  Measured on the way and not kept: the five reloaded X
// values kept (+3.5 % over 97), reads three ahead, the reads as single ds_read_b64 in inline
// assembly with counted lgkmcnt waits.  99 is 98 with the inter-stage twiddles from two
// tables in the workgroup's LDS (kTwLds of acq_kernels.h: the middle stage's powers w^r and
// the last stage's roots, built once per workgroup, read ahead of each stage's barrier --
// no global load left in a transform but the code-row copies, 28 packed products fewer per
// wave; 126 VGPRs, no scratch, occupancy 4, 39,096 B of LDS): +1.2 % over 98 on the C2
// bench, bit-identical results; 98 stays as its A/B partner.  101 is 99 with the correlate's
// transform as the prime-factor 32 x 125 plan (PkPfaPlan4000 of fft_pk.h: the same radices 25,
// 16, 10, no twiddles between the first two stages, the middle stage in place -- 4 barriers per
// transform --, a 2 x 5 last butterfly with 13 twiddle products instead of 21, the roots from
// two small LDS tables, kTwPfa; 122 VGPRs, no scratch, occupancy 4, 33,224 B of LDS).  Forward
// and argmax passes stay on the Stockham plan, and the argmax pass writes the record's peak, so
// the records are variant 70's bit for bit wherever the same Doppler row wins; the row maxima
// differ from 70's by f32 rounding order (tests/test_gpu_acq_pk_prime_factor.py).  +8 % over 99
// on the C2 bench; 99 stays as its A/B partner.  Measured on the way and not kept
// (profiles/pfa101): the powers W_125^(c k) read from a table instead of chained (-2 %).
// 103 is 101 with fewer instructions in the butterflies (PkPfaPlan4000Lean): the 5-point
// transforms of the first stage's radix 25 and of the last stage as DftLean<5>, 16 packed
// instructions instead of 18, and the last stage's outputs 1, 4 and 2, 3 handed to the row
// statistic two at a time, |z|^2 of both in one packed product and one packed fused multiply-add
// (144 of 2029 VALU instructions fewer per transform, LDS traffic and barriers unchanged; 120
// VGPRs, no scratch, occupancy 4).  Other roundings in the row maxima, within the same bound
// against the oracle as 101 (tests/test_gpu_acq_pk_lean_butterflies.py); the records stay the
// argmax pass's.  +2.8 % / +3.3 % over 101 on the C2 bench; 101 stays as its A/B partner.
// Measured on the way and not kept (profiles/lean103): the paired |z|^2 alone on Dft<5>'s own
// values (the old id 102 again; bit-identical row maxima, 56 instructions fewer): +0.3 % /
// +0.4 %, within three times the parent's spread.
template <int ID, class MP, int PG_, int WPE_, int ST, class REG = void, int CS_ = kCodeVgpr, int TW_ = kTwGlobal, class CP = MP>
struct PkVariant
{
    static constexpr int id = ID, PG = PG_, WPE = WPE_, STAT = ST, CS = CS_, TW = TW_;
    using type = MP;
    using Reg = REG;
    using Corr = CP;  // the plan acq_correlate_pk_kernel runs (forward and argmax: type)
    // another plan's row maximum selects the row; the record's peak is the argmax pass's
    static constexpr bool PEAK = !std::is_same<CP, MP>::value;
};
using PkVariants = PlanList<PkVariant<61, PkPlan<512, true, 20, 20, 20>, 1, 1, 1>,
    PkVariant<62, PkPlan<256, true, 20, 10, 10>, 1, 1, 1>,
    PkVariant<93, PkPlan<1024, 1, 16, 10, 10, 10>, 1, 1, 2, RegPlan93>,
    PkVariant<94, PkPlan<1024, 1, 16, 10, 10, 10>, 1, 1, 2, RegPlan94>,
    PkVariant<70, PkPlan<256, 1, 25, 16, 10>, 1, 1, 2>,
    PkVariant<97, PkPlan<256, 1, 25, 16, 10>, 16, 4, 2, void, kCodeLds>,
    PkVariant<98, PkPlan<256, 1, 25, 16, 10>, 16, 4, 2, void, kCodeLane>,
    PkVariant<99, PkPlan<256, 1, 25, 16, 10>, 16, 4, 2, void, kCodeLane, kTwLds>,
    PkVariant<101, PkPlan<256, 1, 25, 16, 10>, 16, 4, 2, void, kCodeLane, kTwPfa, gsdr::pk::PkPfaPlan4000<256>>,
    PkVariant<103, PkPlan<256, 1, 25, 16, 10>, 16, 4, 2, void, kCodeLane, kTwPfa, gsdr::pk::PkPfaPlan4000Lean<256>>>;

// f(PkVariant) -> int for variant id; `unknown` for an id not in the list (an
// internal error in a launch: setup accepted the handle's id).
template <class F>
int with_pk_variant(int id, F&& f, int unknown = GSDR_E_STATE)
{
    int rc = unknown;
    const bool found = find_plan(PkVariants{}, [&](auto e) {
        if (decltype(e)::id != id) return false;
        rc = f(e);
        return true;
    });
    if (!found && unknown != GSDR_OK) gsdr::set_error("internal: bad correlate variant %d", id);
    return rc;
}

}  // namespace

int launch_corr_variant(gsdr_acq* a, const AcqView& v, uint32_t nblocks, hipStream_t s)
{
    return with_pk_variant(a->corr_variant, [&](auto e) {
        using V = decltype(e);
        using M = typename V::type;
        if constexpr (!std::is_void<typename V::Reg>::value)
            {
                using RP = typename V::Reg;
                hipLaunchKernelGGL((acq_correlate_reg_kernel<RP>), dim3(nblocks * v.D * v.nprn), dim3(RP::NT),
                    RP::lds_bytes(), s, a->d_X, v.code_fft, a->d_stats, a->d_tw, v.D, v.nprn, nblocks, v.xm);
            }
        else
            {
                const uint32_t groups = (v.nprn + V::PG - 1) / V::PG;
                hipLaunchKernelGGL((acq_correlate_pk_kernel<typename V::Corr, V::PG, V::WPE, V::STAT, V::CS, V::TW>), dim3(nblocks * v.D * groups),
                    dim3(M::NT), a->corr_lds_bytes, s, a->d_X, V::CS == kCodeLane ? v.code_lane : v.code_fft, a->d_stats, a->d_tw, v.D, v.nprn, nblocks,
                    v.xm);
            }
        return GSDR_OK;
    });
}

// The variants' first-maximum pass over the selected rows.
int launch_argmax_variant(gsdr_acq* a, const AcqView& v, uint32_t nblocks, gsdr_acq_result* res, hipStream_t s)
{
    return with_pk_variant(a->corr_variant, [&](auto e) {
        using V = decltype(e);
        using M = typename V::type;
        hipLaunchKernelGGL((acq_argmax_pk_kernel<M, V::STAT, V::PEAK>), dim3(nblocks * v.nprn), dim3(M::NT), a->corr_lds_bytes,
            s, a->d_X, v.code_fft, res, a->d_tw, v.D, v.nprn, a->conf.samples_per_code, params_of(a, v));
        GSDR_HIP(hipGetLastError());
        return GSDR_OK;
    });
}

// Forward spectra on the packed plan of the selected variant.
int launch_forward_pk(gsdr_acq* a, const AcqView& v, const void* iq, uint32_t nblocks, uint64_t stride, hipStream_t s)
{
    return with_pk_variant(a->corr_variant, [&](auto e) {
        using M = typename decltype(e)::type;
        // a folding view (QuickSync, acq_quicksync.hip): the folding load over items of
        // fold_segments N samples
        with_item_type(a->conf.item_type, [&](auto t) {
            if (v.fold_segments > 0)
                hipLaunchKernelGGL((acq_forward_fold_pk_kernel<M, decltype(t)::value>), dim3(nblocks, v.xm.q),
                    dim3(M::NT), M::lds_bytes(), s, iq, stride, v.wipe, a->d_X, a->d_tw, v.fold_segments, v.xm);
            else
                hipLaunchKernelGGL((acq_forward_pk_kernel<M, decltype(t)::value>), dim3(nblocks, v.xm.q), dim3(M::NT),
                    M::lds_bytes(), s, iq, stride, v.wipe, a->d_X, a->d_tw, a->consumed, v.xm);
        });
        GSDR_HIP(hipGetLastError());
        return GSDR_OK;
    });
}

// Select and configure a correlate variant for the handle's N; an id not in the
// list leaves the generic kernels.
int setup_corr_variant(gsdr_acq* a, int id)
{
    a->corr_variant = 0;
    return with_pk_variant(id, [&](auto e) {
        using V = decltype(e);
        using M = typename V::type;
        if (M::N != (int)a->N)
            {
                gsdr::set_error("correlate variant %d is for N = %d, not %u", V::id, M::N, a->N);
                return GSDR_E_UNSUPPORTED;
            }
        // the correlate's FFT buffer (padded for kCodeLds), two sets of per-wave row statistics and
        // the variant's twiddle tables; the argmax pass, scratch right after its N c2, fits in the
        // same allocation
        using C = typename V::Corr;
        static_assert(C::N == M::N && C::NT == M::NT && C::lds_bytes() >= M::lds_bytes(), "one size, one workgroup, one allocation");
        a->corr_lds_bytes = pk_corr_lds_bytes<C, V::CS, V::TW>();
        int rc = set_max_lds((const void*)acq_correlate_pk_kernel<C, V::PG, V::WPE, V::STAT, V::CS, V::TW>, a->corr_lds_bytes);
        rc |= set_max_lds((const void*)acq_argmax_pk_kernel<M, V::STAT, V::PEAK>, a->corr_lds_bytes);
        for (int it : kItemTypes)
            rc |= with_item_type(it, [&](auto t) {
                return set_max_lds((const void*)acq_forward_pk_kernel<M, decltype(t)::value>, M::lds_bytes()) |
                       set_max_lds((const void*)acq_forward_fold_pk_kernel<M, decltype(t)::value>, M::lds_bytes());
            });
        if constexpr (!std::is_void<typename V::Reg>::value)
            rc |= set_max_lds((const void*)acq_correlate_reg_kernel<typename V::Reg>, V::Reg::lds_bytes());
        if (rc != GSDR_OK) return GSDR_E_DEVICE;
        a->corr_variant = V::id;
        a->lane_nb1 = V::CS == kCodeLane ? C::NB1 : 0;
        a->lane_r1 = V::CS == kCodeLane ? C::R1 : 0;
        a->lane_pfa = V::CS == kCodeLane && C::PRIME_FACTOR ? 1 : 0;
        a->corr_stat = V::STAT;
        return GSDR_OK;
    }, GSDR_OK);
}

}  // namespace gsdr_acq_impl
