// QuickSync acquisition: the launch code and C ABI of gsdr_acq_set_quicksync,
// gsdr_acq_set_quicksync_codes, gsdr_acq_run_quicksync, gsdr_acq_run_quicksync_stream and
// gsdr_acq_dump_quicksync.  The template kernels are in acq_quicksync_kernels.h; the grid
// is the engine's own (the AcqOp::Run sequence on the handle's Nf-point plan, on a view
// whose fold_segments = p^2 selects the folding forward pass and that is first_peak_only).

#include "acq_handle.h"
#include "acq_power_kernel.h"
#include "acq_quicksync_kernels.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

namespace
{

// set_local_code's fold (:146-151): row `slot` of stage (nf points) is the sum of the p
// segments of row `slot` of codes (p nf points).
__global__ void __launch_bounds__(256) acq_quick_code_fold_kernel(const float2* __restrict__ codes,
    float2* __restrict__ stage, uint32_t nf, uint32_t p)
{
    const float2* c = codes + (size_t)blockIdx.x * p * nf;
    float2* out = stage + (size_t)blockIdx.x * nf;
    for (uint32_t i = threadIdx.x; i < nf; i += blockDim.x)
        {
            float2 acc = make_float2(0.f, 0.f);
            for (uint32_t s = 0; s < p; ++s)
                {
                    const float2 v = c[(size_t)s * nf + i];
                    acc.x += v.x;
                    acc.y += v.y;
                }
            out[i] = acc;
        }
}

// One lane per (item b, slot): the record from the slot's grid record, the item's input
// power and the p candidate powers.  index_max over the candidates keeps the first maximum
// (:412); the normalisation divides by (float(Nf) float(Nf))^2 in float (:286, :367).
__global__ void __launch_bounds__(64) acq_quick_merge_kernel(const gsdr_acq_result* __restrict__ slots,
    const float* __restrict__ power, const float* __restrict__ cand, gsdr_acq_quicksync_result* __restrict__ out,
    uint32_t nprn, uint32_t n_records, uint32_t p, uint32_t nf)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_records) return;
    const uint32_t b = i / nprn;
    const gsdr_acq_result w = slots[i];
    const float* c = cand + (size_t)i * p;
    uint32_t best = 0;
    float cmax = c[0];
    for (uint32_t k = 1; k < p; ++k)
        if (c[k] > cmax)
            {
                cmax = c[k];
                best = k;
            }
    const float norm = (float)nf * (float)nf;
    gsdr_acq_quicksync_result r;
    r.prn = w.prn;
    r.doppler_index = w.doppler_index;
    r.folded_phase = w.code_phase;
    r.candidate = best;
    r.doppler_hz = w.doppler_hz;
    r.pad = 0;
    r.mag = w.peak / (norm * norm);
    r.input_power = power[b];
    r.test_statistic = r.mag / r.input_power;
    r.candidate_power = cmax;
    r.acq_delay_samples = (double)(w.code_phase + best * nf);
    r.samplestamp = w.samplestamp;
    out[i] = r;
}

// What a QuickSync call needs of the handle; `who` names the call in the message.
int check_quick_handle(const gsdr_acq* a, const char* who)
{
    const int rc = check_single_grid_handle(a, who, "QuickSync");
    if (rc != GSDR_OK) return rc;
    GSDR_REQUIRE(a->variant < 20, GSDR_E_UNSUPPORTED,
        "%s: fft_size %u runs on a four-step plan; the folding forward transform needs a one-launch LDS plan", who,
        a->N);
    return GSDR_OK;
}

int check_quick_run(const gsdr_acq* a, const char* who)
{
    GSDR_REQUIRE(a->qs.p > 0, GSDR_E_STATE, "%s: gsdr_acq_set_quicksync first", who);
    GSDR_REQUIRE(a->slots == gsdr_acq::Slots::QuickSync, GSDR_E_STATE, "%s: gsdr_acq_set_quicksync_codes first", who);
    GSDR_REQUIRE(a->wipe_mode == GSDR_WIPE_EXACT, GSDR_E_UNSUPPORTED,
        "%s: QuickSync runs with the exact carrier only (gsdr_acq_set_wipeoff mode %d)", who, a->wipe_mode);
    return GSDR_OK;
}

// nitems grids over the active slots at iq (device, items of L at stride L), the input
// powers, the candidate powers and the records into qs.d_out, on the handle's stream.  The
// view carries the run's mode: the rows over an item, the folding forward pass over p^2
// segments (launch_forward, launch_forward_pk) and no second-peak pass (params_of).
int enqueue_quick(gsdr_acq* a, const void* iq, uint32_t nitems, uint64_t stamp0)
{
    gsdr_acq::Quick& q = a->qs;
    hipStream_t s = a->stream;
    const uint64_t L = (uint64_t)q.p * q.spc;
    AcqView v = view_of(a);
    v.wipe = q.d_wipe;
    v.fold_segments = q.p * q.p;
    v.first_peak_only = true;
    const int rc = dispatch(a, v, AcqOp{AcqOp::Run, iq, nitems, L, stamp0, a->d_res, s});
    if (rc != GSDR_OK) return rc;
    StageTimer t(a, s);
    t.begin();
    const uint32_t n = nitems * v.nprn;
    with_item_type(a->conf.item_type, [&](auto it) {
        hipLaunchKernelGGL((acq_pair_power_kernel<decltype(it)::value>), dim3(nitems), dim3(kPairPowerLanes), 0, s, iq, L,
            (uint32_t)L, q.d_power);
        hipLaunchKernelGGL((acq_quick_candidate_kernel<decltype(it)::value>), dim3(n, q.p),
            dim3(kQuickCandLanes), 0, s, iq, L, (const float2*)q.d_wipe, (const float2*)a->d_tw,
            (const float2*)q.d_codes, (const gsdr_acq_result*)a->d_res, q.d_cand, v.nprn, v.D, q.p, q.spc, a->N, v.xm);
    });
    GSDR_HIP(hipGetLastError());
    hipLaunchKernelGGL(acq_quick_merge_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const gsdr_acq_result*)a->d_res,
        (const float*)q.d_power, (const float*)q.d_cand, q.d_out, v.nprn, n, q.p, a->N);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    return GSDR_OK;
}

}  // namespace

void gsdr_acq_impl::quicksync_free(gsdr_acq* a)
{
    gsdr_acq::Quick& q = a->qs;
    void* bufs[] = {q.d_iq, q.d_wipe, q.d_codes, q.d_power, q.d_cand, q.d_out};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    q = gsdr_acq::Quick{};
}

int gsdr_acq_impl::quicksync_rebuild_wipeoffs(gsdr_acq* a)
{
    if (!a->qs.d_wipe) return GSDR_OK;
    // rows 0..q-1 suffice with the reuse, as for the plain grid (rebuild_wipeoffs)
    return launch_wipeoff_long(a, a->qs.d_wipe, a->xm.q, a->qs.p * a->qs.spc);
}

extern "C" {

int gsdr_acq_set_quicksync(gsdr_acq* a, uint32_t folding_factor, uint32_t samples_per_code)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_quicksync: null handle");
    const uint32_t p = folding_factor, spc = samples_per_code;
    // p = 1 would read past the item (delay + spc > L) and p > 100 overrun the reference's
    // accumulators (:385); spc % p != 0 would drop samples from both folds
    GSDR_REQUIRE(p >= 2 && p <= 16, GSDR_E_ARG, "gsdr_acq_set_quicksync: folding factor %u outside [2,16]", p);
    GSDR_REQUIRE(spc > 0 && spc % p == 0, GSDR_E_ARG,
        "gsdr_acq_set_quicksync: samples_per_code %u is no multiple of the folding factor %u", spc, p);
    GSDR_REQUIRE(spc / p == a->N, GSDR_E_ARG,
        "gsdr_acq_set_quicksync: samples_per_code / folding factor = %u, the handle's fft_size is %u", spc / p, a->N);
    int rc = check_quick_handle(a, "gsdr_acq_set_quicksync");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipStreamSynchronize(a->stream));
    quicksync_free(a);
    gsdr_acq::Quick& q = a->qs;
    const size_t L = (size_t)p * spc, nB = a->conf.max_blocks, nP = a->conf.max_prns;
    hipError_t e = hipMalloc(&q.d_iq, nB * L * gsdr::item_bytes(a->conf.item_type));
    if (e == hipSuccess) e = hipMalloc(&q.d_wipe, (size_t)a->D * L * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&q.d_codes, nP * spc * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&q.d_power, nB * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&q.d_cand, nB * nP * p * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&q.d_out, nB * nP * sizeof(gsdr_acq_quicksync_result));
    if (e != hipSuccess)
        {
            quicksync_free(a);
            gsdr::set_error("gsdr_acq_set_quicksync: device allocation failed: %s", hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    q.p = p;
    q.spc = spc;
    rc = quicksync_rebuild_wipeoffs(a);
    if (rc == GSDR_OK && hipStreamSynchronize(a->stream) != hipSuccess) rc = GSDR_E_DEVICE;
    if (rc != GSDR_OK) quicksync_free(a);
    return rc;
}

int gsdr_acq_set_quicksync_codes(gsdr_acq* a, const float* codes, const uint32_t* prn, uint32_t nprn)
{
    GSDR_REQUIRE(a && codes && prn, GSDR_E_ARG, "gsdr_acq_set_quicksync_codes: null argument");
    GSDR_REQUIRE(nprn > 0 && nprn <= a->conf.max_prns, GSDR_E_ARG,
        "gsdr_acq_set_quicksync_codes: nprn %u outside [1,%u]", nprn, a->conf.max_prns);
    std::lock_guard<std::mutex> lk(a->mu);
    GSDR_REQUIRE(a->qs.p > 0, GSDR_E_STATE, "gsdr_acq_set_quicksync_codes: gsdr_acq_set_quicksync first");
    gsdr::DeviceGuard g(a->device);
    gsdr_acq::Quick& q = a->qs;
    // ordered after every launch issued so far on the handle's stream
    GSDR_HIP(hipMemcpyAsync(q.d_codes, codes, (size_t)nprn * q.spc * sizeof(float2), hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->d_prn, prn, nprn * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    // the folds into the staged code rows (consumed == fft_size here); not timed, as the
    // code transform behind it is not
    hipLaunchKernelGGL(acq_quick_code_fold_kernel, dim3(nprn), dim3(256), 0, a->stream, (const float2*)q.d_codes,
        a->d_code_stage, a->N, q.p);
    GSDR_HIP(hipGetLastError());
    const int rc = code_fft(a, 0, nprn);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));  // codes and prn are read until here
    set_slots(a, gsdr_acq::Slots::QuickSync, nprn);
    return GSDR_OK;
}

int gsdr_acq_run_quicksync(gsdr_acq* a, const void* iq_host, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_quicksync_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run_quicksync: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_quicksync", nitems, "nitems");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_quick_run(a, "gsdr_acq_run_quicksync");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    const size_t L = (size_t)a->qs.p * a->qs.spc;
    GSDR_HIP(hipMemcpyAsync(a->qs.d_iq, iq_host, nitems * L * gsdr::item_bytes(a->conf.item_type), hipMemcpyHostToDevice,
        a->stream));
    rc = enqueue_quick(a, a->qs.d_iq, nitems, stamp0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->qs.d_out, (size_t)nitems * a->nprn * sizeof(gsdr_acq_quicksync_result));
}

int gsdr_acq_run_quicksync_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nitems,
    uint64_t stamp0, gsdr_acq_quicksync_result* out)
{
    GSDR_REQUIRE(a && ring && out, GSDR_E_ARG, "gsdr_acq_run_quicksync_stream: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_quicksync_stream", nitems, "nitems");
    if (rc == GSDR_OK)
        rc = gsdr::check_ring_consumer("gsdr_acq_run_quicksync_stream", ring, a->conf.item_type, a->device,
            "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_quick_run(a, "gsdr_acq_run_quicksync_stream");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    rc = with_ring_items(a, ring, first_sample, (uint64_t)nitems * a->qs.p * a->qs.spc,
        [&](const void* iq) { return enqueue_quick(a, iq, nitems, stamp0); });
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->qs.d_out, (size_t)nitems * a->nprn * sizeof(gsdr_acq_quicksync_result));
}

int gsdr_acq_dump_quicksync(gsdr_acq* a, const void* iq_host, float* rows_out, float* cand_out)
{
    GSDR_REQUIRE(a && iq_host, GSDR_E_ARG, "gsdr_acq_dump_quicksync: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    int rc = check_quick_run(a, "gsdr_acq_dump_quicksync");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    const size_t L = (size_t)a->qs.p * a->qs.spc;
    GSDR_HIP(hipMemcpyAsync(a->qs.d_iq, iq_host, L * gsdr::item_bytes(a->conf.item_type), hipMemcpyHostToDevice,
        a->stream));
    // one item's grids; every plan's correlate leaves the row maxima of slot p in
    // stats[p D + d]
    rc = enqueue_quick(a, a->qs.d_iq, 1, 0);
    if (rc != GSDR_OK) return rc;
    if (cand_out)
        GSDR_HIP(hipMemcpyAsync(cand_out, a->qs.d_cand, (size_t)a->nprn * a->qs.p * sizeof(float), hipMemcpyDeviceToHost,
            a->stream));
    const float norm = (float)a->N * (float)a->N;
    if (rows_out) return row_maxima_to_host(a, a->nprn, a->D, norm * norm, rows_out);
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

}  // extern "C"
