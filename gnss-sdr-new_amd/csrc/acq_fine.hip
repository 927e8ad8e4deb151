// Fine-Doppler estimate of the acquisition engine: the second stage of
// pcps_acquisition_fine_doppler_cc (estimate_Doppler, :346-419) for many requests
// on one 10 ms window in one launch.  Kernels in acq_fine_kernels.h.
//
//   K_fine    grid (request, residue r < 8): code wipe-off with the request's aligned
//             replica, the phase ramp of residue r, one L = 10 N point transform on the
//             handle's fine plan (one LDS plan, or the four-step R x N2), |X|^2 and the
//             (maximum, first index) key merged per request by a 64-bit atomic maximum
//   K_finish  per request: fftFreqBins[index], the 1000 Hz test, the result record
#include <cmath>
#include <vector>

#include "acq_fine_kernels.h"
#include "acq_handle.h"
#include "acq_plans.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

namespace
{

constexpr size_t kLdsBytes = 160 * 1024;
// four-step scratch rows (L complex each): a workgroup holds its row only while it
// runs (four_step_claim), so the pool bounds the transforms in flight, not the grid.
// 32 rows (four requests' workgroups at once); the first call with more requests
// grows the pool to 64 rows, its bound.
constexpr int kFineSlots = 32, kFineSlotsMax = 64;

// the pool of `slots` rows (a multiple of 32) in place of the handle's
int fine_set_pool(gsdr_acq* a, gsdr_acq::Fine& f, int slots)
{
    if (a->stream) GSDR_HIP(hipStreamSynchronize(a->stream));
    if (f.d_scratch) (void)hipFree(f.d_scratch);
    if (f.d_slots) (void)hipFree(f.d_slots);
    f.d_scratch = nullptr;
    f.d_slots = nullptr;
    f.plan4.nwords = 0;
    hipError_t e = hipMalloc(&f.d_scratch, (size_t)slots * f.L * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&f.d_slots, (size_t)(slots / 32) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(f.d_slots, 0, (size_t)(slots / 32) * sizeof(uint32_t));
    if (e != hipSuccess)
        {
            gsdr::set_error("fine Doppler: scratch pool of %d rows: %s", slots, hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    f.plan4.nwords = slots / 32;
    f.plan4.scratch = f.d_scratch;
    f.plan4.slots = f.d_slots;
    return GSDR_OK;
}

using FineLds = RuntimePlan<1024>;
using FineFour256 = FourStepPlan<256>;
using FineFour1024 = FourStepPlan<1024>;

// The plan of the handle's L = 10 N point transform (host only, no allocation).
int fine_plan(const gsdr_acq* a, gsdr_acq::Fine& f)
{
    // the block works on 1 ms blocks only (d_fft_size = samples per code, :57-60)
    GSDR_REQUIRE(a->consumed == a->N && !a->conf.bit_transition_flag, GSDR_E_UNSUPPORTED,
        "fine Doppler: needs consumed_samples == fft_size and no bit transition (consumed %u, fft %u, bit transition %d)",
        a->consumed, a->N, a->conf.bit_transition_flag);
    GSDR_REQUIRE(a->N >= 2 && a->N <= (1u << 24) / 80u, GSDR_E_UNSUPPORTED, "fine Doppler: fft_size %u outside [2, %u]",
        a->N, (1u << 24) / 80u);
    const int L = 10 * (int)a->N;
    const auto fits = [](int n) { return (size_t)n * sizeof(float2) + 256 <= kLdsBytes; };
    f = gsdr_acq::Fine{};
    f.L = (uint32_t)L;
    if (fits(L) && gsdr::fft::make_plan(L, FineLds::NT, f.plan) && f.plan.nstages >= 2)
        {
            f.r1 = 0;
            f.nt = FineLds::NT;
            f.lds_bytes = (size_t)L * sizeof(float2);
            return GSDR_OK;
        }
    // four-step L = R * N2: R = 10 first (N2 = N, the sub-transform the coarse stage
    // plans too), else the largest register radix whose N2 has an LDS plan
    const int radices[] = {10, 25, 20, 16, 12, 8};
    const int nts[] = {FineFour256::NT, FineFour1024::NT};
    for (int R : radices)
        {
            if (L % R != 0 || !fits(L / R)) continue;
            for (int nt : nts)
                {
                    Plan sub{};
                    if (!gsdr::fft::make_plan(L / R, nt, sub) || sub.nstages < 2) continue;
                    f.r1 = R;
                    f.nt = nt;
                    f.plan4.n = L;
                    f.plan4.r1 = R;
                    f.plan4.sub = sub;
                    f.plan.n = L;
                    f.lds_bytes = (size_t)sub.n * sizeof(float2);
                    return GSDR_OK;
                }
        }
    gsdr::set_error("fine Doppler: the 10 ms transform of %d points is not supported (needs 2^a*3^b*5^c; up to 20352 "
                    "points in LDS, larger sizes as R*N2 with R in {8,10,12,16,20,25} and N2 <= 20352)", L);
    return GSDR_E_UNSUPPORTED;
}

hipError_t upload_roots(float2* d_tw, uint32_t n)
{
    std::vector<float2> tw(n);
    for (uint32_t m = 0; m < n; ++m)
        {
            const double ang = 2.0 * M_PI * (double)m / (double)n;
            tw[m] = make_float2((float)std::cos(ang), (float)(-std::sin(ang)));
        }
    return hipMemcpy(d_tw, tw.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice);
}

template <class PT>
int fine_set_attrs(size_t bytes)
{
    int rc = GSDR_OK;
    for (int it : kItemTypes)
        rc |= with_item_type(it, [&](auto t) {
            return set_max_lds((const void*)acq_fine_kernel<PT, decltype(t)::value>, bytes);
        });
    return rc == GSDR_OK ? GSDR_OK : GSDR_E_DEVICE;
}

template <class PT>
void fine_launch_on(gsdr_acq* a, const void* iq, uint32_t nreq, float* spec)
{
    const gsdr_acq::Fine& f = a->fine;
    const typename PT::PlanT* plan;
    if constexpr (std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        plan = &f.plan4;
    else
        plan = &f.plan;
    with_item_type(a->conf.item_type, [&](auto t) {
        hipLaunchKernelGGL((acq_fine_kernel<PT, decltype(t)::value>), dim3(nreq, 8), dim3(PT::NT), f.lds_bytes,
            a->stream, iq, (const float2*)f.d_codes, (const gsdr_acq_fine_request*)f.d_req, f.d_keys, spec,
            (const float2*)f.d_tw, *plan, a->N);
        return 0;
    });
}

void free_fine_buffers(gsdr_acq::Fine& f)
{
    void* bufs[] = {f.d_tw, f.d_tw_sub, f.d_scratch, f.d_slots, f.d_iq, f.d_codes, f.d_req, f.d_out, f.d_keys, f.d_spec};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    f = gsdr_acq::Fine{};
}

// Device copies of the call's code rows and requests, the zeroed keys, the two
// launches: everything up to the result records in d_out, on the handle's stream.
int fine_enqueue(gsdr_acq* a, const void* iq_dev, const float* codes, uint32_t ncodes,
    const gsdr_acq_fine_request* reqs, uint32_t nreq, float* spec)
{
    gsdr_acq::Fine& f = a->fine;
    if (f.r1 > 0 && nreq * 8u > (uint32_t)f.plan4.nwords * 32u && f.plan4.nwords * 32 < kFineSlotsMax)
        {
            const int rc = fine_set_pool(a, f, kFineSlotsMax);
            if (rc != GSDR_OK)
                {
                    // no pool: the plan is rebuilt by the next call
                    free_fine_buffers(f);
                    return rc;
                }
        }
    if (ncodes > f.codes_cap)
        {
            GSDR_HIP(hipStreamSynchronize(a->stream));
            if (f.d_codes) (void)hipFree(f.d_codes);
            f.d_codes = nullptr;
            f.codes_cap = 0;
            GSDR_HIP(hipMalloc(&f.d_codes, (size_t)ncodes * a->N * sizeof(float2)));
            f.codes_cap = ncodes;
        }
    if (nreq > f.req_cap)
        {
            GSDR_HIP(hipStreamSynchronize(a->stream));
            void** bufs[] = {(void**)&f.d_req, (void**)&f.d_out, (void**)&f.d_keys};
            for (void** p : bufs)
                {
                    if (*p) (void)hipFree(*p);
                    *p = nullptr;
                }
            f.req_cap = 0;
            GSDR_HIP(hipMalloc(&f.d_req, (size_t)nreq * sizeof(gsdr_acq_fine_request)));
            GSDR_HIP(hipMalloc(&f.d_out, (size_t)nreq * sizeof(gsdr_acq_fine_result)));
            GSDR_HIP(hipMalloc(&f.d_keys, (size_t)nreq * sizeof(unsigned long long)));
            f.req_cap = nreq;
        }
    GSDR_HIP(hipMemcpyAsync(f.d_codes, codes, (size_t)ncodes * a->N * sizeof(float2), hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(f.d_req, reqs, (size_t)nreq * sizeof(gsdr_acq_fine_request), hipMemcpyHostToDevice,
        a->stream));
    GSDR_HIP(hipMemsetAsync(f.d_keys, 0, (size_t)nreq * sizeof(unsigned long long), a->stream));
    GSDR_HIP(hipMemsetAsync(f.d_out, 0, (size_t)nreq * sizeof(gsdr_acq_fine_result), a->stream));
    // gsdr_acq_set_profiling: K_fine as stage 0 (the transform), K_finish as stage 2
    StageTimer t(a, a->stream);
    t.begin();
    if (f.r1 == 0)
        fine_launch_on<FineLds>(a, iq_dev, nreq, spec);
    else if (f.nt == FineFour256::NT)
        fine_launch_on<FineFour256>(a, iq_dev, nreq, spec);
    else
        fine_launch_on<FineFour1024>(a, iq_dev, nreq, spec);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    t.begin();
    hipLaunchKernelGGL(acq_fine_finish_kernel, dim3((nreq + 63) / 64), dim3(64), 0, a->stream,
        (const unsigned long long*)f.d_keys, (const gsdr_acq_fine_request*)f.d_req, f.d_out, nreq,
        (float)a->conf.fs_in, 8u * f.L);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    return GSDR_OK;
}

int check_requests(const gsdr_acq* a, const char* who, const gsdr_acq_fine_request* reqs, uint32_t nreq, uint32_t ncodes)
{
    GSDR_REQUIRE(nreq > 0 && ncodes > 0, GSDR_E_ARG, "%s: %u requests on %u code rows", who, nreq, ncodes);
    for (uint32_t i = 0; i < nreq; ++i)
        {
            GSDR_REQUIRE(reqs[i].code_phase < a->N, GSDR_E_ARG, "%s: request %u: code_phase %u >= fft_size %u", who, i,
                reqs[i].code_phase, a->N);
            GSDR_REQUIRE(reqs[i].code_slot < ncodes, GSDR_E_ARG, "%s: request %u: code_slot %u >= ncodes %u", who, i,
                reqs[i].code_slot, ncodes);
        }
    return GSDR_OK;
}

}  // namespace

int gsdr_acq_impl::fine_prepare(gsdr_acq* a)
{
    if (a->fine.ready) return GSDR_OK;
    gsdr_acq::Fine f;
    int rc = fine_plan(a, f);
    if (rc != GSDR_OK) return rc;
    if (f.r1 == 0)
        rc = fine_set_attrs<FineLds>(f.lds_bytes);
    else if (f.nt == FineFour256::NT)
        rc = fine_set_attrs<FineFour256>(f.lds_bytes);
    else
        rc = fine_set_attrs<FineFour1024>(f.lds_bytes);
    if (rc != GSDR_OK) return rc;
    hipError_t e = hipMalloc(&f.d_tw, (size_t)f.L * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&f.d_iq, (size_t)f.L * gsdr::item_bytes(a->conf.item_type));
    if (e == hipSuccess && f.r1 > 0)
        {
            e = hipMalloc(&f.d_tw_sub, (size_t)f.plan4.sub.n * sizeof(float2));
            if (e == hipSuccess) e = upload_roots(f.d_tw_sub, (uint32_t)f.plan4.sub.n);
            f.plan4.tw_sub = f.d_tw_sub;
            if (e == hipSuccess && fine_set_pool(a, f, kFineSlots) != GSDR_OK) e = hipErrorOutOfMemory;
        }
    if (e == hipSuccess) e = upload_roots(f.d_tw, f.L);
    if (e != hipSuccess)
        {
            free_fine_buffers(f);
            gsdr::set_error("fine Doppler: device allocation failed: %s", hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    f.ready = true;
    a->fine = f;
    return GSDR_OK;
}

void gsdr_acq_impl::fine_free(gsdr_acq* a) { free_fine_buffers(a->fine); }

extern "C" {

int gsdr_acq_get_fine_plan(const gsdr_acq* a, uint32_t* L, int32_t* r1, uint32_t* n2)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_get_fine_plan: null handle");
    gsdr_acq::Fine f;
    const int rc = fine_plan(a, f);
    if (rc != GSDR_OK) return rc;
    if (L) *L = f.L;
    if (r1) *r1 = f.r1;
    if (n2) *n2 = f.r1 > 0 ? (uint32_t)f.plan4.sub.n : f.L;
    return GSDR_OK;
}

int gsdr_acq_get_fine_ready(gsdr_acq* a, int32_t* ready)
{
    GSDR_REQUIRE(a && ready, GSDR_E_ARG, "gsdr_acq_get_fine_ready: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    *ready = a->fine.ready ? 1 : 0;
    return GSDR_OK;
}

int gsdr_acq_fine_doppler(gsdr_acq* a, const void* iq_host, const float* codes, uint32_t ncodes,
    const gsdr_acq_fine_request* requests, uint32_t nreq, gsdr_acq_fine_result* out)
{
    GSDR_REQUIRE(a && iq_host && codes && requests && out, GSDR_E_ARG, "gsdr_acq_fine_doppler: null argument");
    int rc = check_requests(a, "gsdr_acq_fine_doppler", requests, nreq, ncodes);
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    rc = fine_prepare(a);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(a->fine.d_iq, iq_host, (size_t)a->fine.L * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    rc = fine_enqueue(a, a->fine.d_iq, codes, ncodes, requests, nreq, nullptr);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->fine.d_out, (size_t)nreq * sizeof(gsdr_acq_fine_result));
}

int gsdr_acq_fine_doppler_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, const float* codes,
    uint32_t ncodes, const gsdr_acq_fine_request* requests, uint32_t nreq, gsdr_acq_fine_result* out_host)
{
    GSDR_REQUIRE(a && ring && codes && requests && out_host, GSDR_E_ARG, "gsdr_acq_fine_doppler_stream: null argument");
    int rc = check_requests(a, "gsdr_acq_fine_doppler_stream", requests, nreq, ncodes);
    if (rc != GSDR_OK) return rc;
    rc = gsdr::check_ring_consumer("gsdr_acq_fine_doppler_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    rc = fine_prepare(a);
    if (rc != GSDR_OK) return rc;
    rc = with_ring_items(a, ring, first_sample, a->fine.L, [&](const void* iq) {
        return fine_enqueue(a, iq, codes, ncodes, requests, nreq, nullptr);
    });
    if (rc != GSDR_OK) return rc;
    return read_back(a, out_host, a->fine.d_out, (size_t)nreq * sizeof(gsdr_acq_fine_result));
}

int gsdr_acq_dump_fine_spectrum(gsdr_acq* a, const void* iq_host, const float* code, uint32_t code_phase,
    float* spectrum_host)
{
    GSDR_REQUIRE(a && iq_host && code && spectrum_host, GSDR_E_ARG, "gsdr_acq_dump_fine_spectrum: null argument");
    const gsdr_acq_fine_request rq{code_phase, 0.0f, 0u};
    int rc = check_requests(a, "gsdr_acq_dump_fine_spectrum", &rq, 1, 1);
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr::DeviceGuard g(a->device);
    rc = fine_prepare(a);
    if (rc != GSDR_OK) return rc;
    gsdr_acq::Fine& f = a->fine;
    const size_t M = (size_t)8 * f.L;
    if (!f.d_spec) GSDR_HIP(hipMalloc(&f.d_spec, M * sizeof(float)));
    GSDR_HIP(hipMemcpyAsync(f.d_iq, iq_host, (size_t)f.L * gsdr::item_bytes(a->conf.item_type), hipMemcpyHostToDevice,
        a->stream));
    rc = fine_enqueue(a, f.d_iq, code, 1, &rq, 1, f.d_spec);
    if (rc != GSDR_OK) return rc;
    return read_back(a, spectrum_host, f.d_spec, M * sizeof(float));
}

}  // extern "C"
