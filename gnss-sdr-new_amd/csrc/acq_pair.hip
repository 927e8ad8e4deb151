// Paired-code acquisition: the launch code and C ABI of gsdr_acq_set_code_pairs,
// gsdr_acq_run_pairs, gsdr_acq_run_pairs_stream and gsdr_acq_dump_pair_rows.  The kernels
// are in acq_pair_kernels.h; the transforms are the engine's own (the AcqOp::Run
// sequence over two code slots per pair, on a view marked first_peak_only).
#include <vector>

#include "acq_handle.h"
#include "acq_pair_kernels.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

namespace
{

// What a pair run needs of the handle; `who` names the call in the message.
int check_pair_run(const gsdr_acq* a, const char* who)
{
    const int rc = check_single_grid_handle(a, who, "pairs");
    if (rc != GSDR_OK) return rc;
    GSDR_REQUIRE(a->slots == gsdr_acq::Slots::Pairs, GSDR_E_STATE, "%s: gsdr_acq_set_code_pairs first", who);
    return GSDR_OK;
}

int pairs_prepare(gsdr_acq* a)
{
    gsdr_acq::Pairs& p = a->pairs;
    if (p.d_in) return GSDR_OK;
    const size_t maxpairs = a->conf.max_prns / 2;
    hipError_t e = hipMalloc(&p.d_power, (size_t)a->conf.max_blocks * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&p.d_out, (size_t)a->conf.max_blocks * maxpairs * sizeof(gsdr_acq_pair_result));
    if (e == hipSuccess) e = hipMalloc(&p.d_in, 2 * maxpairs * a->N * sizeof(float2));
    if (e != hipSuccess)
        {
            pairs_free(a);
            gsdr::set_error("gsdr_acq_set_code_pairs: device allocation failed: %s", hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    return GSDR_OK;
}

// nblocks grids over the nprn = 2 npairs slots at iq (device), the input powers and the
// merged records into pairs.d_out, on the handle's stream.  A pair reads no second peak:
// the view is first_peak_only.
int enqueue_pairs(gsdr_acq* a, const void* iq, uint32_t nblocks, uint64_t stamp0)
{
    hipStream_t s = a->stream;
    AcqView v = view_of(a);
    v.first_peak_only = true;
    const int rc = dispatch(a, v, AcqOp{AcqOp::Run, iq, nblocks, a->consumed, stamp0, a->d_res, s});
    if (rc != GSDR_OK) return rc;
    const uint32_t npairs = v.nprn / 2;
    StageTimer t(a, s);
    t.begin();
    with_item_type(a->conf.item_type, [&](auto it) {
        hipLaunchKernelGGL((acq_pair_power_kernel<decltype(it)::value>), dim3(nblocks), dim3(kPairPowerLanes), 0, s, iq,
            (uint64_t)a->consumed, a->N, a->pairs.d_power);
    });
    GSDR_HIP(hipGetLastError());
    const uint32_t n = nblocks * npairs;
    hipLaunchKernelGGL(acq_pair_merge_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const gsdr_acq_result*)a->d_res,
        (const float*)a->pairs.d_power, a->pairs.d_out, npairs, n, (float)a->N,
        (uint32_t)a->conf.samples_per_code);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    return GSDR_OK;
}

}  // namespace

void gsdr_acq_impl::pairs_free(gsdr_acq* a)
{
    gsdr_acq::Pairs& p = a->pairs;
    if (p.d_in) (void)hipFree(p.d_in);
    if (p.d_power) (void)hipFree(p.d_power);
    if (p.d_out) (void)hipFree(p.d_out);
    p.d_in = nullptr;
    p.d_power = nullptr;
    p.d_out = nullptr;
}

extern "C" {

int gsdr_acq_set_code_pairs(gsdr_acq* a, int kind, const float* first, const float* second, const uint32_t* prn,
    uint32_t npairs)
{
    GSDR_REQUIRE(a && first && second && prn, GSDR_E_ARG, "gsdr_acq_set_code_pairs: null argument");
    GSDR_REQUIRE(kind == GSDR_ACQ_PAIR_AS_IS || kind == GSDR_ACQ_PAIR_SUM_DIFF_J, GSDR_E_ARG,
        "gsdr_acq_set_code_pairs: unknown kind %d", kind);
    GSDR_REQUIRE(npairs > 0 && 2ull * npairs <= a->conf.max_prns, GSDR_E_ARG,
        "gsdr_acq_set_code_pairs: %u pairs need %llu code slots, the handle has %u", npairs, 2ull * npairs,
        a->conf.max_prns);
    int rc = check_single_grid_handle(a, "gsdr_acq_set_code_pairs", "pairs");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    rc = pairs_prepare(a);
    if (rc != GSDR_OK) return rc;
    const size_t row = (size_t)a->N * sizeof(float2);
    float2* d_first = a->pairs.d_in;
    float2* d_second = a->pairs.d_in + (size_t)npairs * a->N;
    std::vector<uint32_t> ids(2 * (size_t)npairs);
    for (uint32_t q = 0; q < npairs; ++q) ids[2 * q] = ids[2 * q + 1] = prn[q];
    // ordered after every launch issued so far on the handle's stream
    GSDR_HIP(hipMemcpyAsync(d_first, first, npairs * row, hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(d_second, second, npairs * row, hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->d_prn, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    // the members into the staged code rows (consumed == fft_size here); not timed, as
    // the code transform behind it is not
    hipLaunchKernelGGL(acq_pair_replica_kernel, dim3(npairs), dim3(256), 0, a->stream, (const float2*)d_first,
        (const float2*)d_second, a->d_code_stage, a->N, kind);
    GSDR_HIP(hipGetLastError());
    rc = code_fft(a, 0, 2 * npairs);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));  // ids is read until here
    set_slots(a, gsdr_acq::Slots::Pairs, 2 * npairs);
    return GSDR_OK;
}

int gsdr_acq_run_pairs(gsdr_acq* a, const void* iq_host, uint32_t nblocks, uint64_t stamp0, gsdr_acq_pair_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run_pairs: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_pairs", nblocks, "nblocks");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_pair_run(a, "gsdr_acq_run_pairs");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)nblocks * a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    rc = enqueue_pairs(a, a->d_iq, nblocks, stamp0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->pairs.d_out, (size_t)nblocks * (a->nprn / 2) * sizeof(gsdr_acq_pair_result));
}

int gsdr_acq_run_pairs_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nblocks, uint64_t stamp0,
    gsdr_acq_pair_result* out)
{
    GSDR_REQUIRE(a && ring && out, GSDR_E_ARG, "gsdr_acq_run_pairs_stream: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_pairs_stream", nblocks, "nblocks");
    if (rc == GSDR_OK)
        rc = gsdr::check_ring_consumer("gsdr_acq_run_pairs_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_pair_run(a, "gsdr_acq_run_pairs_stream");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    rc = with_ring_items(a, ring, first_sample, (uint64_t)nblocks * a->consumed,
        [&](const void* iq) { return enqueue_pairs(a, iq, nblocks, stamp0); });
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->pairs.d_out, (size_t)nblocks * (a->nprn / 2) * sizeof(gsdr_acq_pair_result));
}

int gsdr_acq_dump_pair_rows(gsdr_acq* a, const void* iq_host, float* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_dump_pair_rows: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    int rc = check_pair_run(a, "gsdr_acq_dump_pair_rows");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->consumed * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    // one block's grids; every plan's correlate leaves the row maxima of slot p in
    // stats[p D + d]
    rc = enqueue_pairs(a, a->d_iq, 1, 0);
    if (rc != GSDR_OK) return rc;
    const float norm = (float)a->N * (float)a->N;
    return row_maxima_to_host(a, a->nprn, a->D, norm * norm, out);
}

}  // extern "C"
