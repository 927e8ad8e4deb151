// PCPS acquisition engine for MI355X (gfx950).
//
// Restates pcps_acquisition::acquisition_core
// (src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.cc:615-882) as a
// batched grid over (block, Doppler bin, PRN):
//
//   K_wipe    (init)  w_d[n] = exp(j*phi_n), phi accumulated in fp32 exactly like the
//                     generic volk_gnsssdr_s32f_sincos_32fc (pcps_acquisition.cc:233-246,298-305)
//   K_code    (init)  Cf_p = FFT(code_p placed in the FFT buffer)       (:176-209)
//   K_forward         X_{b,d} = FFT(x_b .* w_d)                          (:658-662)
//   K_correlate       per (b,d,p): |IFFT(X_{b,d} .* conj(Cf_p))|^2 in LDS, fused with the
//                     row reductions (max, first argmax, sum); the D x N magnitude grid
//                     of the reference never reaches HBM                  (:664-679)
//   K_reduce          per (b,p): grid maximum with the reference tie-break, CFAR input power,
//                     Gnss_Synchro fields                                (:511-543, :697-713)
//   K_second          per (b,p), peak-ratio mode only: recompute row d*, second peak outside
//                     the +-1 chip window with the reference's wrap      (:546-612)
//
//   K_quick   QuickSync (pcps_quicksync_acquisition_cc): the folded code, the folding forward
//                     transform in place of K_forward, the item's input power and the check of
//                     the p delays the folded winner stands for (acq_quicksync.hip)
//   K_tong    Tong (pcps_tong_acquisition_cc): the grid accumulated over a sequence of items, each
//                     scaled by its own input power, walked by one workgroup per row, and the
//                     counter over the items' maxima (acq_tong.hip)
//   K_pair    paired codes (pcps_cccwsr_acquisition_cc, galileo_pcps_8ms_acquisition_cc): the
//                     two replicas of a pair, the block's input power and the merge of a
//                     pair's two slot records, around the kernels above (acq_pair.hip)
//
// This unit is the C ABI.  The kernels are in acq_kernels.h / acq_split_kernels.h
// (templates) and acq_common.hip, the launch sequences in acq_launch.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <utility>

#include "acq_handle.h"
#include "acq_plans.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

int gsdr_acq_impl::dispatch(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    if (a->variant >= 20) return dispatch_four(a, v, op);
    if (a->variant >= 10) return dispatch_runtime(a, v, op);
    return dispatch_static(a, v, op);
}

int gsdr_acq_impl::code_fft(gsdr_acq* a, uint32_t first_slot, uint32_t nslots)
{
    AcqOp op{AcqOp::CodeFft};
    op.first_slot = first_slot;
    op.nslots = nslots;
    const int rc = dispatch(a, view_of(a), op);
    // the refreshed slots' lane-order copies, behind their spectra on the handle's stream
    if (rc != GSDR_OK || !a->d_code_lane) return rc;
    return launch_code_lane_order(a, first_slot, nslots);
}

namespace
{

// AcqOp::Run of nblocks blocks at iq (device), results to res (device).
int run_blocks(gsdr_acq* a, const AcqView& v, const void* iq, uint32_t nblocks, uint64_t stride, uint64_t stamp0,
    gsdr_acq_result* res, hipStream_t s)
{
    return dispatch(a, v, AcqOp{AcqOp::Run, iq, nblocks, stride, stamp0, res, s});
}

// The same on the ring's samples from first_sample, into d_res on the handle's stream.
int run_ring(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nblocks, uint64_t stamp0)
{
    return with_ring_items(a, ring, first_sample, (uint64_t)nblocks * a->K * a->consumed, [&](const void* iq) {
        return run_blocks(a, view_of(a), iq, nblocks, a->consumed, stamp0, a->d_res, a->stream);
    });
}

// update_grid_doppler_wipeoffs_step2 (pcps_acquisition.cc:307-314), float arithmetic:
// the nb frequencies of a narrow grid around center
void step_two_freqs(const gsdr_acq* a, float center, float* freqs)
{
    const uint32_t nb = a->st2.nbins;
    const float half = (float)std::floor((double)nb / 2.0);
    for (uint32_t d = 0; d < nb; ++d)
        {
            volatile float dop = ((float)d - half) * a->st2.step;
            freqs[d] = center + dop;
        }
}

// The table W_n^m = exp(-2 pi i m / n), m < n, in double, rounded once.
hipError_t upload_twiddles(float2* d_tw, uint32_t n)
{
    std::vector<float2> tw(n);
    for (uint32_t m = 0; m < n; ++m)
        {
            const double ang = 2.0 * M_PI * (double)m / (double)n;
            tw[m] = make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
        }
    return hipMemcpy(d_tw, tw.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice);
}

// Pick a compile-time plan when one matches N, else the smallest workgroup that
// admits a runtime plan, else a four-step plan (acq_plans.h).

void set_four(gsdr_acq* a, int id, int nt, int r1, const Plan& sub)
{
    a->variant = id;
    a->nt = nt;
    a->plan4 = gsdr::fft::Plan4{};
    a->plan4.n = (int)a->N;
    a->plan4.r1 = r1;
    a->plan4.sub = sub;
    a->plan.n = (int)a->N;  // buffer sizes
}

bool choose_variant(gsdr_acq* a)
{
    const int N = (int)a->N;
    const auto fits = [](int n) { return (size_t)n * sizeof(float2) + 16 * sizeof(RowStat) <= kLdsBytes; };
    if (find_plan(StaticPlans{}, [&](auto e) {
            using PT = typename decltype(e)::type;
            if (PT::N != N) return false;
            a->variant = e.id;
            a->nt = PT::NT;
            a->plan = PT::plan();
            return true;
        }))
        return true;
    if (find_plan(RuntimePlans{}, [&](auto e) {
            using PT = typename decltype(e)::type;
            if (!gsdr::fft::make_plan(N, PT::NT, a->plan) || a->plan.nstages < 2 || !fits(N)) return false;
            a->variant = e.id;
            a->nt = PT::NT;
            return true;
        }))
        return true;
    // the packed four-step at its sizes
    if (!a->env.four_generic && find_plan(FourPkPlans{}, [&](auto e) {
            using PT = typename decltype(e)::type;
            if (PT::N != N) return false;
            Plan sub{};
            sub.n = PT::N2;
            sub.nstages = 0;  // compile-time sub-plan
            set_four(a, e.id, PT::NT, PT::R, sub);
            return true;
        }))
        return true;
    // four-step (fft_4step.h): N = R * N2, the largest register radix R whose N2
    // has an LDS plan
    const int radices[] = {25, 20, 16, 12, 10, 8};
    for (int R : radices)
        {
            if (N % R != 0 || !fits(N / R)) continue;
            if (find_plan(FourPlans{}, [&](auto e) {
                    using PT = typename decltype(e)::type;
                    Plan sub{};
                    if (!gsdr::fft::make_plan(N / R, PT::NT, sub) || sub.nstages < 2) return false;
                    set_four(a, e.id, PT::NT, R, sub);
                    return true;
                }))
                return true;
        }
    return false;
}

}  // namespace

// ====================================================================== ABI
extern "C" {

int gsdr_acq_create(int device, const gsdr_acq_conf* conf, gsdr_acq** out)
{
    GSDR_REQUIRE(conf && out, GSDR_E_ARG, "gsdr_acq_create: null argument");
    *out = nullptr;
    GSDR_REQUIRE(conf->fs_in > 0 && conf->consumed_samples > 0, GSDR_E_ARG, "gsdr_acq_create: fs_in and consumed_samples must be > 0");
    GSDR_REQUIRE(conf->doppler_step > 0, GSDR_E_ARG, "gsdr_acq_create: doppler_step must be > 0");
    GSDR_REQUIRE(conf->item_type == GSDR_ITEM_GR_COMPLEX || conf->item_type == GSDR_ITEM_CSHORT ||
                     conf->item_type == GSDR_ITEM_IBYTE, GSDR_E_ARG,
        "gsdr_acq_create: unknown item type %d", conf->item_type);
    GSDR_REQUIRE(conf->max_prns > 0 && conf->max_blocks > 0, GSDR_E_ARG, "gsdr_acq_create: capacities must be > 0");
    GSDR_REQUIRE(conf->pfa >= 0.0f && conf->pfa <= 1.0f, GSDR_E_ARG, "gsdr_acq_create: pfa outside [0,1]");
    int ndev = 0;
    GSDR_HIP(hipGetDeviceCount(&ndev));
    GSDR_REQUIRE(device >= 0 && device < ndev, GSDR_E_ARG, "gsdr_acq_create: device %d of %d", device, ndev);
    gsdr::DeviceGuard g(device);

    gsdr_acq* a = new (std::nothrow) gsdr_acq();
    GSDR_REQUIRE(a, GSDR_E_ALLOC, "gsdr_acq_create: out of host memory");
    std::unique_ptr<gsdr_acq, void (*)(gsdr_acq*)> guard(a, gsdr_acq_destroy);  // until *out takes it
    a->device = device;
    a->conf = *conf;
    if (a->conf.max_dwells == 0) a->conf.max_dwells = 1;
    // bit transition: every call decides on its own (the dwell counter is reset,
    // pcps_acquisition.cc:871-879) and the threshold uses one dwell (:908)
    if (a->conf.bit_transition_flag) a->conf.max_dwells = 1;
    a->K = a->conf.max_dwells;
    a->consumed = conf->consumed_samples;
    a->env = read_acq_env();
    a->wipe_mode = a->env.wipe_mode;
    // pcps_acquisition.cc:85-92
    uint32_t N = conf->fft_size;
    if (N == 0) N = (conf->sampled_ms == conf->ms_per_code || conf->sampled_ms == 0) ? a->consumed : 2 * a->consumed;
    GSDR_REQUIRE(N >= a->consumed, GSDR_E_ARG, "gsdr_acq_create: fft_size %u < consumed_samples %u", N, a->consumed);
    a->N = N;
    a->lead = N - a->consumed;
    a->eff = N;
    if (conf->bit_transition_flag)
        {
            GSDR_REQUIRE(N % 2 == 0, GSDR_E_ARG, "gsdr_acq_create: bit_transition_flag needs an even fft_size (%u)", N);
            a->lead = N / 2;
            a->eff = N / 2;
        }
    a->general = a->K > 1 || conf->bit_transition_flag;
    a->D = conf->num_doppler_bins;
    if (a->D == 0)
        a->D = (uint32_t)std::ceil((double)(conf->doppler_max - (-conf->doppler_max)) / (double)conf->doppler_step);
    GSDR_REQUIRE(a->D != 0, GSDR_E_ARG, "gsdr_acq_create: zero Doppler bins");
    const bool ok = choose_variant(a);
    const bool four = a->variant >= 20;
    a->lds_bytes = (size_t)(four ? a->plan4.sub.n : N) * sizeof(float2) + 16 * sizeof(RowStat);
    GSDR_REQUIRE(ok && a->lds_bytes <= kLdsBytes, GSDR_E_UNSUPPORTED,
        "gsdr_acq_create: FFT size %u not supported (needs 2^a*3^b*5^c; up to 20352 points in LDS, larger sizes as "
        "R*N2 with R in {8,10,12,16,20,25} and N2 <= 20352)", N);
    int rc = dispatch(a, view_of(a), AcqOp{AcqOp::SetAttrs});
    if (rc == GSDR_OK && four) rc = setup_split(a);
    if (rc == GSDR_OK && !a->general && default_pk_variant(N) > 0)
        rc = setup_corr_variant(a, a->env.corr_variant >= 0 ? a->env.corr_variant : default_pk_variant(N));
    if (rc != GSDR_OK) return rc;
    const size_t nP = conf->max_prns, nB = conf->max_blocks;
    hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&a->d_tw, (size_t)N * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&a->d_wipe, (size_t)a->D * N * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&a->d_code_fft, nP * N * sizeof(float2));
    if (e == hipSuccess && a->lane_nb1 > 0) e = hipMalloc(&a->d_code_lane, nP * N * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&a->d_code_stage, nP * a->consumed * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&a->d_prn, nP * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&a->d_X, nB * a->K * a->D * N * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&a->d_stats, nB * nP * a->K * a->D * sizeof(RowStat));
    if (e == hipSuccess) e = hipMalloc(&a->d_res, nB * nP * sizeof(gsdr_acq_result));
    if (e == hipSuccess) e = hipMalloc(&a->d_iq, nB * a->K * a->consumed * gsdr::item_bytes(conf->item_type));
    if (a->general)
        {
            // accumulation rows held by resident workgroups only: the chip's resident
            // workgroup count bounds the pool
            const int nslots = 256 * 32 / (a->nt / 64);
            a->acc_words = (nslots + 31) / 32;
            if (e == hipSuccess) e = hipMalloc(&a->d_resk, nB * nP * a->K * sizeof(gsdr_acq_result));
            if (e == hipSuccess) e = hipMalloc(&a->d_acc, (size_t)a->acc_words * 32 * a->eff * sizeof(float));
            if (e == hipSuccess) e = hipMalloc(&a->d_acc_slots, (size_t)a->acc_words * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMemset(a->d_acc_slots, 0, (size_t)a->acc_words * sizeof(uint32_t));
        }
    if (e == hipSuccess) e = hipMalloc(&a->d_grid, (size_t)a->D * N * sizeof(float));
    // split path with the peak-ratio statistic: one |R|^2 row per (block, PRN) for the
    // merged first/second-peak pass (acq_argmax_second_four_kernel)
    if (e == hipSuccess && a->split > 0 && !(conf->pfa > 0.0f))
        e = hipMalloc(&a->d_rowbuf, nB * nP * N * sizeof(float));
    // split path: the selected rows' first-maximum keys (acq_correlate_split_kernel<ARG>)
    if (e == hipSuccess && a->split > 0) e = hipMalloc(&a->d_keys, nB * nP * sizeof(unsigned long long));
    if (e == hipSuccess && a->split > 0) e = hipMalloc(&a->d_psum, nB * nP * 4 * sizeof(float));
    // split path: the two-launch forward's scratch rows (columns on every CU, then rows:
    // +8-12 % on C4 / C5 over one workgroup per spectrum, r04e)
    if (e == hipSuccess && a->split > 0) e = hipMalloc(&a->d_fscratch, nB * a->K * a->D * N * sizeof(float2));
    if (four)
        {
            // scratch slots: at least the resident workgroup count of the chip
            // (256 CUs x 32 waves / waves per workgroup), capped at 4 GiB
            int nslots = 256 * 32 / (a->nt / 64);
            while (nslots > 64 && (size_t)nslots * N * sizeof(float2) > (4ull << 30)) nslots /= 2;
            nslots = (nslots + 31) / 32 * 32;
            a->plan4.nwords = nslots / 32;
            if (e == hipSuccess) e = hipMalloc(&a->d_tw_sub, (size_t)a->plan4.sub.n * sizeof(float2));
            if (e == hipSuccess) e = hipMalloc(&a->d_scratch, (size_t)nslots * N * sizeof(float2));
            if (e == hipSuccess) e = hipMalloc(&a->d_slots, (size_t)a->plan4.nwords * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMemset(a->d_slots, 0, (size_t)a->plan4.nwords * sizeof(uint32_t));
            if (e == hipSuccess) e = upload_twiddles(a->d_tw_sub, (uint32_t)a->plan4.sub.n);
            a->plan4.tw_sub = a->d_tw_sub;
            a->plan4.scratch = a->d_scratch;
            a->plan4.slots = a->d_slots;
        }
    GSDR_REQUIRE(e == hipSuccess, GSDR_E_ALLOC, "gsdr_acq_create: device allocation failed: %s", hipGetErrorString(e));
    e = upload_twiddles(a->d_tw, N);
    GSDR_REQUIRE(e == hipSuccess, GSDR_E_DEVICE, "gsdr_acq_create: twiddle upload: %s", hipGetErrorString(e));
    rc = rebuild_wipeoffs(a);
    if (rc != GSDR_OK) return rc;
    compute_threshold(a);
    // GSDR_ACQ_FINE=1: the fine-Doppler plan and buffers now instead of on the first
    // call; a size it does not cover stays a valid handle (that call reports it)
    const char* fine_env = std::getenv("GSDR_ACQ_FINE");
    if (fine_env && fine_env[0] == '1' && fine_env[1] == '\0')
        {
            rc = fine_prepare(a);
            if (rc != GSDR_OK && rc != GSDR_E_UNSUPPORTED) return rc;
        }
    *out = guard.release();
    return GSDR_OK;
}

void gsdr_acq_destroy(gsdr_acq* a)
{
    if (!a) return;
    gsdr::DeviceGuard g(a->device);
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    for (auto& r : a->prof_recs)
        {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
    for (hipEvent_t e : a->prof_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < gsdr_acq::kSubs; ++i)
        {
            if (a->sub_done[i]) (void)hipEventDestroy(a->sub_done[i]);
            if (a->h_res[i]) (void)hipHostFree(a->h_res[i]);
        }
    void* bufs[] = {a->st2.d_wipe, a->st2.d_freq, a->d_tw, a->d_wipe, a->d_code_fft, a->d_code_lane, a->d_code_stage, a->d_prn, a->d_X, a->d_stats, a->d_res,
        a->d_iq, a->d_grid, a->d_rowbuf, a->d_keys, a->d_psum, a->d_fscratch, a->d_dgrid, a->d_tw_sub, a->d_scratch, a->d_slots, a->d_resk, a->d_acc, a->d_acc_slots};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    fine_free(a);
    pairs_free(a);
    quicksync_free(a);
    tong_free(a);
    iqcaf_free(a);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

int gsdr_acq_get_dims(const gsdr_acq* a, uint32_t* D, uint32_t* N)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_get_dims: null handle");
    if (D) *D = a->D;
    if (N) *N = a->N;
    return GSDR_OK;
}

int gsdr_acq_get_plan(const gsdr_acq* a, int32_t* variant, int32_t* nthreads, int32_t* r1, int32_t* nstages,
    int32_t radix[8])
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_get_plan: null handle");
    static_assert(gsdr::fft::kMaxStages == 8, "gsdr_acq_get_plan reports 8 radices");
    const bool four = a->variant >= 20;
    const Plan& p = four ? a->plan4.sub : a->plan;
    if (variant) *variant = a->variant;
    if (nthreads) *nthreads = a->nt;
    if (r1) *r1 = four ? a->plan4.r1 : 0;
    if (nstages) *nstages = p.nstages;
    if (radix)
        for (int i = 0; i < gsdr::fft::kMaxStages; ++i) radix[i] = i < p.nstages ? p.radix[i] : 1;
    return GSDR_OK;
}

int gsdr_acq_get_split(const gsdr_acq* a, int32_t* split)
{
    GSDR_REQUIRE(a && split, GSDR_E_ARG, "gsdr_acq_get_split: null argument");
    *split = a->split;
    return GSDR_OK;
}

int gsdr_acq_set_local_codes(gsdr_acq* a, const float* codes, const uint32_t* prn, uint32_t nprn)
{
    GSDR_REQUIRE(a && codes && prn, GSDR_E_ARG, "gsdr_acq_set_local_codes: null argument");
    GSDR_REQUIRE(nprn > 0 && nprn <= a->conf.max_prns, GSDR_E_ARG, "gsdr_acq_set_local_codes: nprn %u outside [1,%u]",
        nprn, a->conf.max_prns);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_code_stage, codes, (size_t)nprn * a->consumed * sizeof(float2),
        hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->d_prn, prn, nprn * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    int rc = code_fft(a, 0, nprn);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));
    set_slots(a, gsdr_acq::Slots::Plain, nprn);
    return GSDR_OK;
}

int gsdr_acq_set_local_code(gsdr_acq* a, uint32_t slot, const float* code, uint32_t prn)
{
    GSDR_REQUIRE(a && code, GSDR_E_ARG, "gsdr_acq_set_local_code: null argument");
    GSDR_REQUIRE(slot < a->conf.max_prns, GSDR_E_ARG, "gsdr_acq_set_local_code: slot %u outside [0,%u)",
        slot, a->conf.max_prns);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    // ordered after every launch issued so far on the handle's stream (the slot's
    // previous spectrum may still be read by a submitted grid)
    GSDR_HIP(hipMemcpyAsync(a->d_code_stage + (size_t)slot * a->consumed, code, (size_t)a->consumed * sizeof(float2),
        hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->d_prn + slot, &prn, sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    int rc = code_fft(a, slot, 1);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));
    set_slots(a, gsdr_acq::Slots::Plain, std::max(a->nprn, slot + 1));
    return GSDR_OK;
}

int gsdr_acq_set_active_prns(gsdr_acq* a, uint32_t nprn)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_active_prns: null handle");
    GSDR_REQUIRE(nprn > 0 && nprn <= a->conf.max_prns, GSDR_E_ARG, "gsdr_acq_set_active_prns: %u outside [1,%u]", nprn,
        a->conf.max_prns);
    std::lock_guard<std::mutex> lk(a->mu);
    set_slots(a, gsdr_acq::Slots::Plain, nprn);
    return GSDR_OK;
}

int gsdr_acq_set_doppler(gsdr_acq* a, int32_t doppler_max, uint32_t doppler_step, int32_t doppler_center)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_doppler: null handle");
    GSDR_REQUIRE(doppler_step > 0, GSDR_E_ARG, "gsdr_acq_set_doppler: doppler_step must be > 0");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    const uint32_t D = (uint32_t)std::ceil((double)(doppler_max - (-doppler_max)) / (double)doppler_step);
    GSDR_REQUIRE(a->conf.num_doppler_bins != 0 || D == a->D, GSDR_E_UNSUPPORTED,
        "gsdr_acq_set_doppler: changing the number of Doppler bins (%u -> %u) requires a new handle", a->D, D);
    a->conf.doppler_max = doppler_max;
    a->conf.doppler_step = doppler_step;
    a->conf.doppler_center = doppler_center;
    int rc = rebuild_wipeoffs(a);
    if (rc != GSDR_OK) return rc;
    compute_threshold(a);
    return GSDR_OK;
}

int gsdr_acq_set_wipeoff(gsdr_acq* a, int mode)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_wipeoff: null handle");
    GSDR_REQUIRE(mode == GSDR_WIPE_EXACT || mode == GSDR_WIPE_GENERIC || mode == GSDR_WIPE_AVX2, GSDR_E_ARG,
        "gsdr_acq_set_wipeoff: unknown mode %d", mode);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    a->wipe_mode = mode;
    return rebuild_wipeoffs(a);
}

int gsdr_acq_get_spectrum_reuse(const gsdr_acq* a, uint32_t* q, uint32_t* p)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_get_spectrum_reuse: null handle");
    if (q) *q = a->xm.q;
    if (p) *p = a->xm.p;
    return GSDR_OK;
}

int gsdr_acq_set_threshold(gsdr_acq* a, float threshold)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_threshold: null handle");
    a->threshold = threshold;
    return GSDR_OK;
}

int gsdr_acq_get_threshold(const gsdr_acq* a, float* threshold)
{
    GSDR_REQUIRE(a && threshold, GSDR_E_ARG, "gsdr_acq_get_threshold: null argument");
    *threshold = a->threshold;
    return GSDR_OK;
}

int gsdr_acq_run_device(gsdr_acq* a, const void* iq_dev, uint32_t nblocks, uint64_t stride, uint64_t stamp0,
    gsdr_acq_result* out_dev, void* stream)
{
    GSDR_REQUIRE(a && iq_dev && out_dev, GSDR_E_ARG, "gsdr_acq_run_device: null argument");
    GSDR_REQUIRE(a->nprn > 0 && a->slots != gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "gsdr_acq_run_device: set_local_codes first");
    int rc = check_block_count(a, "gsdr_acq_run_device", nblocks, "nblocks");
    if (rc != GSDR_OK) return rc;
    GSDR_REQUIRE(stride >= a->consumed || nblocks == 1, GSDR_E_ARG, "gsdr_acq_run_device: block stride %llu < consumed %u",
        (unsigned long long)stride, a->consumed);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    hipStream_t s = stream ? (hipStream_t)stream : a->stream;
    return run_blocks(a, view_of(a), iq_dev, nblocks, stride, stamp0, out_dev, s);
}

int gsdr_acq_run(gsdr_acq* a, const void* iq_host, uint32_t nblocks, uint64_t stamp0, gsdr_acq_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run: null argument");
    GSDR_REQUIRE(a->nprn > 0 && a->slots != gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "gsdr_acq_run: set_local_codes first");
    int rc = check_block_count(a, "gsdr_acq_run", nblocks, "nblocks");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    const size_t bytes = (size_t)nblocks * a->K * a->consumed * gsdr::item_bytes(a->conf.item_type);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, bytes, hipMemcpyHostToDevice, a->stream));
    rc = run_blocks(a, view_of(a), a->d_iq, nblocks, a->consumed, stamp0, a->d_res, a->stream);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->d_res, (size_t)nblocks * a->nprn * sizeof(gsdr_acq_result));
}

int gsdr_acq_run_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nblocks, uint64_t stamp0,
    gsdr_acq_result* out)
{
    GSDR_REQUIRE(a && ring && out, GSDR_E_ARG, "gsdr_acq_run_stream: null argument");
    GSDR_REQUIRE(a->nprn > 0 && a->slots != gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "gsdr_acq_run_stream: set_local_codes first");
    int rc = check_block_count(a, "gsdr_acq_run_stream", nblocks, "nblocks");
    if (rc == GSDR_OK) rc = gsdr::check_ring_consumer("gsdr_acq_run_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    rc = run_ring(a, ring, first_sample, nblocks, stamp0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->d_res, (size_t)nblocks * a->nprn * sizeof(gsdr_acq_result));
}

int gsdr_acq_submit_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nblocks, uint64_t stamp0)
{
    GSDR_REQUIRE(a && ring, GSDR_E_ARG, "gsdr_acq_submit_stream: null argument");
    GSDR_REQUIRE(a->nprn > 0 && a->slots != gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "gsdr_acq_submit_stream: set_local_codes first");
    int rc = check_block_count(a, "gsdr_acq_submit_stream", nblocks, "nblocks");
    if (rc == GSDR_OK) rc = gsdr::check_ring_consumer("gsdr_acq_submit_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    GSDR_REQUIRE(a->sub_count < gsdr_acq::kSubs, GSDR_E_STATE,
        "gsdr_acq_submit_stream: %d submissions in flight, collect the oldest first", gsdr_acq::kSubs);
    gsdr::DeviceGuard g(a->device);
    const int slot = (a->sub_head + a->sub_count) % gsdr_acq::kSubs;
    if (!a->h_res[slot])
        {
            GSDR_HIP(hipHostMalloc(&a->h_res[slot],
                (size_t)a->conf.max_blocks * a->conf.max_prns * sizeof(gsdr_acq_result), hipHostMallocDefault));
            GSDR_HIP(hipEventCreateWithFlags(&a->sub_done[slot], hipEventDisableTiming));
        }
    rc = run_ring(a, ring, first_sample, nblocks, stamp0);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(a->h_res[slot], a->d_res, (size_t)nblocks * a->nprn * sizeof(gsdr_acq_result),
        hipMemcpyDeviceToHost, a->stream));
    GSDR_HIP(hipEventRecord(a->sub_done[slot], a->stream));
    a->sub_blocks[slot] = nblocks;
    a->sub_nprn[slot] = a->nprn;
    a->sub_count++;
    return GSDR_OK;
}

int gsdr_acq_collect(gsdr_acq* a, gsdr_acq_result* out, uint32_t* nblocks, uint32_t* nprn)
{
    GSDR_REQUIRE(a && out, GSDR_E_ARG, "gsdr_acq_collect: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    GSDR_REQUIRE(a->sub_count > 0, GSDR_E_STATE, "gsdr_acq_collect: nothing submitted");
    gsdr::DeviceGuard g(a->device);
    const int slot = a->sub_head;
    a->sub_head = (a->sub_head + 1) % gsdr_acq::kSubs;
    a->sub_count--;
    GSDR_HIP(hipEventSynchronize(a->sub_done[slot]));
    std::memcpy(out, a->h_res[slot], (size_t)a->sub_blocks[slot] * a->sub_nprn[slot] * sizeof(gsdr_acq_result));
    if (nblocks) *nblocks = a->sub_blocks[slot];
    if (nprn) *nprn = a->sub_nprn[slot];
    return GSDR_OK;
}

int gsdr_acq_run_dwell(gsdr_acq* a, const void* iq_host, uint32_t dwell, uint64_t stamp, gsdr_acq_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run_dwell: null argument");
    GSDR_REQUIRE(a->nprn > 0 && a->slots != gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "gsdr_acq_run_dwell: set_local_codes first");
    GSDR_REQUIRE(dwell < a->conf.max_dwells, GSDR_E_ARG, "gsdr_acq_run_dwell: dwell %u outside [0,%u)", dwell,
        a->conf.max_dwells);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    if (!a->d_dgrid)
        GSDR_HIP(hipMalloc(&a->d_dgrid, (size_t)a->conf.max_prns * a->D * a->eff * sizeof(float)));
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    AcqOp op{AcqOp::Dwell};
    op.dwell = dwell;
    op.stamp0 = stamp;
    op.res = a->d_res;
    op.s = a->stream;
    int rc = dispatch(a, view_of(a), op);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->d_res, a->nprn * sizeof(gsdr_acq_result));
}

int gsdr_acq_dump_spectra(gsdr_acq* a, const void* iq_host, float* spectra_host)
{
    GSDR_REQUIRE(a && iq_host && spectra_host, GSDR_E_ARG, "gsdr_acq_dump_spectra: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    int rc = dispatch(a, view_of(a), AcqOp{AcqOp::DumpSpectra});
    if (rc != GSDR_OK) return rc;
    // row d of block 0 wherever the layout keeps it (XMap: a window of a shared spectrum)
    for (uint32_t d = 0; d < a->D; ++d)
        GSDR_HIP(hipMemcpyAsync(spectra_host + (size_t)d * a->N * 2, a->d_X + a->xm.off(0, d),
            (size_t)a->N * sizeof(float2), hipMemcpyDeviceToHost, a->stream));
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

int gsdr_acq_dump_grid(gsdr_acq* a, const void* iq_host, uint32_t prn_slot, float* grid_host)
{
    GSDR_REQUIRE(a && iq_host && grid_host, GSDR_E_ARG, "gsdr_acq_dump_grid: null argument");
    GSDR_REQUIRE(prn_slot < a->nprn, GSDR_E_ARG, "gsdr_acq_dump_grid: prn_slot %u >= nprn %u", prn_slot, a->nprn);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    AcqOp op{AcqOp::DumpGrid};
    op.prn_slot = prn_slot;
    int rc = dispatch(a, view_of(a), op);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(grid_host, a->d_grid, (size_t)a->D * a->N * sizeof(float), hipMemcpyDeviceToHost,
        a->stream));
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

int gsdr_acq_dump_row_maxima(gsdr_acq* a, const void* iq_host, float* out_host)
{
    GSDR_REQUIRE(a && iq_host && out_host, GSDR_E_ARG, "gsdr_acq_dump_row_maxima: null argument");
    GSDR_REQUIRE(a->nprn > 0, GSDR_E_STATE, "gsdr_acq_dump_row_maxima: set_local_codes first");
    GSDR_REQUIRE(a->corr_variant > 0 && !a->general && a->split == 0, GSDR_E_UNSUPPORTED,
        "gsdr_acq_dump_row_maxima: the handle runs no packed correlate variant");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    const AcqView v = view_of(a);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    int rc = launch_forward_pk(a, v, a->d_iq, 1, a->consumed, a->stream);
    if (rc == GSDR_OK) rc = launch_corr_variant(a, v, 1, a->stream);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipGetLastError());
    return row_maxima_to_host(a, v.nprn, v.D, 1.0f, out_host);
}

int gsdr_acq_dump_grid_step_two(gsdr_acq* a, const void* iq_host, uint32_t prn_slot, float doppler_center_hz,
    float* grid_host)
{
    GSDR_REQUIRE(a && iq_host && grid_host, GSDR_E_ARG, "gsdr_acq_dump_grid_step_two: null argument");
    GSDR_REQUIRE(prn_slot < a->nprn, GSDR_E_ARG, "gsdr_acq_dump_grid_step_two: prn_slot %u >= nprn %u", prn_slot,
        a->nprn);
    GSDR_REQUIRE(a->st2.nbins > 0, GSDR_E_STATE, "gsdr_acq_dump_grid_step_two: gsdr_acq_set_step_two first");
    GSDR_REQUIRE(a->st2.nbins <= a->D, GSDR_E_UNSUPPORTED,
        "gsdr_acq_dump_grid_step_two: %u narrow bins exceed the grid buffer's %u rows", a->st2.nbins, a->D);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    const uint32_t nb = a->st2.nbins;
    std::vector<float> freqs(nb);
    step_two_freqs(a, doppler_center_hz, freqs.data());
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->st2.d_freq, freqs.data(), nb * sizeof(float), hipMemcpyHostToDevice, a->stream));
    int rc = launch_wipeoff(a, a->st2.d_wipe, nb, a->st2.d_freq);
    if (rc != GSDR_OK) return rc;
    // the grid dump on a one-PRN view with the narrow Doppler rows (plain layout)
    AcqView v = view_of(a);
    v.D = nb;
    v.nprn = 1;
    v.wipe = a->st2.d_wipe;
    v.code_fft = a->d_code_fft + (size_t)prn_slot * a->N;
    v.code_lane = a->d_code_lane ? a->d_code_lane + (size_t)prn_slot * a->N : nullptr;
    v.xm = XMap{nb, 0u, a->N};
    rc = dispatch(a, v, AcqOp{AcqOp::DumpGrid});
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(grid_host, a->d_grid, (size_t)nb * a->N * sizeof(float), hipMemcpyDeviceToHost,
        a->stream));
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

int gsdr_acq_set_step_two(gsdr_acq* a, uint32_t num_doppler_bins_step2, float doppler_step2, float pfa2)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_step_two: null handle");
    GSDR_REQUIRE(num_doppler_bins_step2 > 0, GSDR_E_ARG, "gsdr_acq_set_step_two: zero bins");
    GSDR_REQUIRE(num_doppler_bins_step2 <= a->D * a->conf.max_blocks, GSDR_E_UNSUPPORTED,
        "gsdr_acq_set_step_two: %u bins exceed the handle's spectrum capacity (%u bins x %u blocks)",
        num_doppler_bins_step2, a->D, a->conf.max_blocks);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipStreamSynchronize(a->stream));
    if (a->st2.d_wipe) (void)hipFree(a->st2.d_wipe);
    if (a->st2.d_freq) (void)hipFree(a->st2.d_freq);
    a->st2.d_wipe = nullptr;
    a->st2.d_freq = nullptr;
    const size_t rows = (size_t)a->conf.max_prns * num_doppler_bins_step2;
    GSDR_HIP(hipMalloc(&a->st2.d_wipe, rows * a->N * sizeof(float2)));
    GSDR_HIP(hipMalloc(&a->st2.d_freq, rows * sizeof(float)));
    a->st2.nbins = num_doppler_bins_step2;
    a->st2.step = doppler_step2;
    // Acq_Conf: pfa_second_step outside (0, 1] falls back to pfa (acq_conf.cc:72-76)
    a->st2.pfa2 = (pfa2 <= 0.0f || pfa2 > 1.0f) ? a->conf.pfa : pfa2;
    return GSDR_OK;
}

int gsdr_acq_get_step_two_threshold(const gsdr_acq* a, float* threshold)
{
    GSDR_REQUIRE(a && threshold, GSDR_E_ARG, "gsdr_acq_get_step_two_threshold: null argument");
    GSDR_REQUIRE(a->st2.nbins > 0, GSDR_E_STATE, "gsdr_acq_get_step_two_threshold: gsdr_acq_set_step_two first");
    *threshold = step_two_threshold(a);
    return GSDR_OK;
}

int gsdr_acq_run_step_two(gsdr_acq* a, const void* iq_host, uint32_t nsel, const uint32_t* prn_slots,
    const float* doppler_center_hz, const float* coarse_input_power, uint64_t stamp, gsdr_acq_result* out)
{
    GSDR_REQUIRE(a && iq_host && prn_slots && doppler_center_hz && coarse_input_power && out, GSDR_E_ARG,
        "gsdr_acq_run_step_two: null argument");
    GSDR_REQUIRE(a->st2.nbins > 0, GSDR_E_STATE, "gsdr_acq_run_step_two: gsdr_acq_set_step_two first");
    GSDR_REQUIRE(nsel > 0 && nsel <= a->nprn, GSDR_E_ARG, "gsdr_acq_run_step_two: %u PRNs outside [1,%u]", nsel,
        a->nprn);
    for (uint32_t i = 0; i < nsel; ++i)
        GSDR_REQUIRE(prn_slots[i] < a->nprn, GSDR_E_ARG, "gsdr_acq_run_step_two: slot %u >= nprn %u", prn_slots[i],
            a->nprn);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    const uint32_t nb = a->st2.nbins;
    std::vector<float> freqs((size_t)nsel * nb);
    for (uint32_t i = 0; i < nsel; ++i) step_two_freqs(a, doppler_center_hz[i], freqs.data() + (size_t)i * nb);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->K * a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->st2.d_freq, freqs.data(), freqs.size() * sizeof(float), hipMemcpyHostToDevice,
        a->stream));
    int rc = launch_wipeoff(a, a->st2.d_wipe, nsel * nb, a->st2.d_freq);
    // one narrow grid per PRN (each has its own centre): the engine's launches on a
    // one-PRN view with that PRN's rows, plain layout and step-two parameters
    const float thr = step_two_threshold(a);
    for (uint32_t i = 0; i < nsel && rc == GSDR_OK; ++i)
        {
            AcqView v;
            v.D = nb;
            v.nprn = 1;
            v.wipe = a->st2.d_wipe + (size_t)i * nb * a->N;
            v.code_fft = a->d_code_fft + (size_t)prn_slots[i] * a->N;
            v.code_lane = a->d_code_lane ? a->d_code_lane + (size_t)prn_slots[i] * a->N : nullptr;
            v.prn = a->d_prn + prn_slots[i];
            v.xm = XMap{nb, 0u, a->N};
            v.step_two = true;
            v.center2 = doppler_center_hz[i];
            v.ip2 = coarse_input_power[i];
            v.threshold2 = thr;
            rc = run_blocks(a, v, a->d_iq, 1, a->consumed, stamp, a->d_res + i, a->stream);
        }
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->d_res, nsel * sizeof(gsdr_acq_result));
}

int gsdr_acq_set_cu_mask(gsdr_acq* a, const uint32_t* mask, int n_words)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_cu_mask: null handle");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    return gsdr::replace_stream(&a->stream, mask, n_words);
}

int gsdr_acq_set_profiling(gsdr_acq* a, int enable)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_profiling: null handle");
    std::lock_guard<std::mutex> lk(a->mu);
    a->profiling = enable != 0;
    if (a->profiling)
        {
            // pre-create the stage events, so a profiled run records pooled events
            // instead of calling hipEventCreate inside the caller's timed loop (8 per
            // call: four stages bracketed; read_profile returns them to the pool)
            gsdr::DeviceGuard g(a->device);
            while (a->prof_pool.size() + 2 * a->prof_recs.size() < 1024)
                {
                    hipEvent_t e = nullptr;
                    if (hipEventCreate(&e) != hipSuccess) break;
                    a->prof_pool.push_back(e);
                }
        }
    return GSDR_OK;
}

int gsdr_acq_read_profile_ex(gsdr_acq* a, double* stage_ms, uint32_t* launches, double* stage_busy_ms)
{
    GSDR_REQUIRE(a && stage_ms && launches, GSDR_E_ARG, "gsdr_acq_read_profile: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    for (int i = 0; i < 4; ++i)
        {
            stage_ms[i] = 0.0;
            launches[i] = 0;
            if (stage_busy_ms) stage_busy_ms[i] = 0.0;
        }
    // per launch: duration, and [start, end) against the first record's start event
    std::vector<std::pair<double, double>> iv[4];
    hipEvent_t ref = a->prof_recs.empty() ? nullptr : a->prof_recs.front().a;
    for (auto& r : a->prof_recs)
        {
            GSDR_HIP(hipEventSynchronize(r.b));
            float ms = 0.0f, t0 = 0.0f, t1 = 0.0f;
            GSDR_HIP(hipEventElapsedTime(&ms, r.a, r.b));
            GSDR_HIP(hipEventElapsedTime(&t0, ref, r.a));
            GSDR_HIP(hipEventElapsedTime(&t1, ref, r.b));
            stage_ms[r.stage] += ms;
            launches[r.stage] += 1;
            iv[r.stage].emplace_back(t0, t1);
        }
    // busy time of a stage: the union of its launch intervals (launches of one stage
    // overlap when runs of the handle are issued on several streams)
    if (stage_busy_ms)
        for (int i = 0; i < 4; ++i)
            {
                std::sort(iv[i].begin(), iv[i].end());
                double busy = 0.0, lo = 0.0, hi = -1e300;
                for (const auto& x : iv[i])
                    {
                        if (x.first > hi)
                            {
                                if (hi > lo) busy += hi - lo;
                                lo = x.first;
                                hi = x.second;
                            }
                        else if (x.second > hi)
                            hi = x.second;
                    }
                if (hi > lo) busy += hi - lo;
                stage_busy_ms[i] = busy;
            }
    for (auto& r : a->prof_recs)
        {
            a->prof_pool.push_back(r.a);
            a->prof_pool.push_back(r.b);
        }
    a->prof_recs.clear();
    return GSDR_OK;
}

int gsdr_acq_read_profile_intervals(gsdr_acq* a, const void* ref_event, int stage, double* start_ms, double* end_ms,
    uint32_t max_n, uint32_t* n)
{
    GSDR_REQUIRE(a && ref_event && n && (max_n == 0 || (start_ms && end_ms)), GSDR_E_ARG,
        "gsdr_acq_read_profile_intervals: null argument");
    GSDR_REQUIRE(stage >= 0 && stage < 4, GSDR_E_ARG, "gsdr_acq_read_profile_intervals: stage %d", stage);
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    hipEvent_t ref = (hipEvent_t)const_cast<void*>(ref_event);
    uint32_t k = 0;
    for (auto& r : a->prof_recs)
        {
            if (r.stage != stage) continue;
            if (k < max_n)
                {
                    GSDR_HIP(hipEventSynchronize(r.b));
                    float t0 = 0.0f, t1 = 0.0f;
                    GSDR_HIP(hipEventElapsedTime(&t0, ref, r.a));
                    GSDR_HIP(hipEventElapsedTime(&t1, ref, r.b));
                    start_ms[k] = t0;
                    end_ms[k] = t1;
                }
            ++k;
        }
    *n = k;
    return GSDR_OK;
}

int gsdr_acq_read_profile(gsdr_acq* a, double* stage_ms, uint32_t* launches)
{
    return gsdr_acq_read_profile_ex(a, stage_ms, launches, nullptr);
}

}  // extern "C"
