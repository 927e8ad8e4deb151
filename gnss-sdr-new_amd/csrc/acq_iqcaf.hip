// E5a non-coherent IQ acquisition with CAF filter: the launch code and C ABI of
// gsdr_acq_set_iq_caf, gsdr_acq_set_iq_codes, gsdr_acq_run_iq_caf, gsdr_acq_run_iq_caf_stream and
// gsdr_acq_dump_iq_caf_rows.  The grid kernel template is in acq_iqcaf_kernels.h and is launched
// through the per-plan dispatch (AcqOp::IqCaf, acq_launch.h) on a view that carries the run's
// buffers; the kernels that are no templates are here.

#include <vector>

#include "acq_handle.h"
#include "acq_power_kernel.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

namespace
{

// ---------------------------------------------------------------- K_iqcaf_replica
// The staged code rows of satellite q = blockIdx.x, slots q nslots + (I-A, [I-B], [Q-A], [Q-B]),
// from the caller's rows code_i[q] and code_q[q] of n complex each: an A form is the row as it
// is, a B form the row with its first spc samples negated (set_local_code, :186-205: the product
// with gr_complex(-1, 0) over d_samples_per_code samples of the FFT's input buffer, which still
// holds the A form).
__global__ void __launch_bounds__(256) acq_iqcaf_replica_kernel(const float2* __restrict__ code_i,
    const float2* __restrict__ code_q, float2* __restrict__ stage, uint32_t n, uint32_t spc, uint32_t has_b,
    uint32_t both)
{
    const uint32_t q = blockIdx.x, nslots = (has_b ? 2u : 1u) * (both ? 2u : 1u);
    float2* out = stage + (size_t)q * nslots * n;
    const float2* ci = code_i + (size_t)q * n;
    const float2* cq = code_q + (size_t)q * n;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        {
            const float2 a = ci[i];
            // (-1 + 0 j)(x + y j) = (-x - 0 y) + (0 x - y) j: the sign of both parts
            const float2 na = make_float2(-a.x, -a.y);
            uint32_t s = 0;
            out[(size_t)(s++) * n + i] = a;
            if (has_b) out[(size_t)(s++) * n + i] = i < spc ? na : a;
            if (both)
                {
                    const float2 b = cq[i];
                    out[(size_t)(s++) * n + i] = b;
                    if (has_b) out[(size_t)(s++) * n + i] = i < spc ? make_float2(-b.x, -b.y) : b;
                }
        }
}

struct CafParams
{
    int32_t half;  // CAF_bins_half (0: the filter is off)
    uint32_t both;
};

// d_CAF_vector[di] of :609-667 over the chosen peaks of the D row records at r: float sums in
// the reference's order, every product and sum rounded on its own, the three loops with their
// own divisors, the signed (doppler_index - i) where the reference has it and abs where it has
// that, and the Q term added after its own division.
__device__ float caf_value(const gsdr_acq_iq_caf_row* __restrict__ r, int D, int half, bool both, int di)
{
#pragma clang fp contract(off)
    const float w = 0.5f / (float)half;
    const float fh = (float)half;
    float vi = 0.0f, vq = 0.0f;
    if (di < half)
        {
            const float fd = (float)di;
            for (int i = 0; i < half + di + 1; ++i) vi += r[i].peak_i * (1.0f - w * (float)(di - i));
            vi /= 1.0f + (float)(half + di) - w * fh * ((fh + 1.0f) / 2.0f) - w * fd * (fd + 1.0f) / 2.0f;
            if (both)
                {
                    for (int i = 0; i < half + di + 1; ++i) vq += r[i].peak_q * (1.0f - w * (float)abs(di - i));
                    vq /= 1.0f + (float)(half + di) - w * fh * (float)(half + 1) / 2.0f - w * fd * (float)(di + 1) / 2.0f;
                }
        }
    else if (di < D - half)
        {
            const float div = 1.0f + 2.0f * fh - 2.0f * w * fh * (float)(half + 1) / 2.0f;
            for (int i = di - half; i < di + half + 1; ++i) vi += r[i].peak_i * (1.0f - w * (float)(di - i));
            vi /= div;
            if (both)
                {
                    for (int i = di - half; i < di + half + 1; ++i) vq += r[i].peak_q * (1.0f - w * (float)(di - i));
                    vq /= div;
                }
        }
    else
        {
            const float fr = (float)(D - di - 1), fr1 = (float)(D - di);
            for (int i = di - half; i < D; ++i) vi += r[i].peak_i * (1.0f - w * (float)abs(di - i));
            vi /= 1.0f + fh + fr - w * fh * (fh + 1.0f) / 2.0f - w * fr * fr1 / 2.0f;
            if (both)
                {
                    for (int i = di - half; i < D; ++i) vq += r[i].peak_q * (1.0f - w * (float)abs(di - i));
                    // :664 divides by the double 2.0: the differences are taken in double and the
                    // divisor rounded to float once
                    const double dv = (double)(1.0f + fh + fr) - (double)(w * fh * (float)((double)half + 1.0)) / 2.0 -
                                      (double)(w * fr * fr1) / 2.0;
                    vq /= (float)dv;
                }
        }
    return both ? vi + vq : vi;
}

// ---------------------------------------------------------------- K_iqcaf_finish
// One wave per (item k, satellite): blockIdx.x = k nsat + sat.  The winner over the D row records
// is the first row, rows ascending, whose quotient sum_peak / (fn fn) is above every earlier one
// (d_mag < magt from d_mag = 0, :549): the largest quotient, the smallest row among equals, and
// none where every quotient is 0 -- the record then keeps the zeros set_state(1) wrote.  With the
// filter on, lane di computes d_CAF_vector[di] and the first maximum names caf_doppler_index
// (:670).
__global__ void __launch_bounds__(64) acq_iqcaf_finish_kernel(const gsdr_acq_iq_caf_row* __restrict__ rec,
    const float* __restrict__ power, const uint32_t* __restrict__ prn, gsdr_acq_iq_caf_result* __restrict__ out,
    AcqParams ap, uint32_t nsat, uint32_t nslots, uint32_t spc, CafParams cp, uint64_t stamp0)
{
    const uint32_t b = blockIdx.x, k = b / nsat, sat = b - k * nsat, lane = threadIdx.x;
    const gsdr_acq_iq_caf_row* r = rec + (size_t)b * ap.D;
    const float fn = gsdr::mul_rn((float)ap.N, (float)ap.N);
    const float fn2 = gsdr::mul_rn(fn, fn);
    float best = 0.0f, cbest = -1.0f;
    uint32_t brow = 0xffffffffu, bidx = 0, crow = 0xffffffffu;
    for (uint32_t d = lane; d < ap.D; d += 64)
        {
            const float magt = r[d].sum_peak / fn2;
            if (stat_better(magt, d, best, brow))
                {
                    best = magt;
                    brow = d;
                    bidx = r[d].sum_index;
                }
            if (cp.half > 0)
                {
                    const float c = caf_value(r, (int)ap.D, cp.half, cp.both != 0, (int)d);
                    if (stat_better(c, d, cbest, crow))
                        {
                            cbest = c;
                            crow = d;
                        }
                }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            const float om = __shfl_xor(best, off), oc = __shfl_xor(cbest, off);
            const uint32_t orow = __shfl_xor(brow, off), oidx = __shfl_xor(bidx, off), ocrow = __shfl_xor(crow, off);
            if (stat_better(om, orow, best, brow))
                {
                    best = om;
                    brow = orow;
                    bidx = oidx;
                }
            if (stat_better(oc, ocrow, cbest, crow))
                {
                    cbest = oc;
                    crow = ocrow;
                }
        }
    if (lane != 0) return;
    gsdr_acq_iq_caf_result o{};
    o.prn = prn[sat * nslots];
    o.samplestamp = stamp0 + (uint64_t)k * ap.N;
    o.input_power = power[k];
    // a row wins only with a quotient above 0 (stat_better's tie at 0 went to the smaller row)
    if (best > 0.0f)
        {
            o.doppler_index = brow;
            o.indext = bidx;
            o.doppler_hz = doppler_of(ap, brow);
            o.acq_delay_samples = (double)(bidx % spc);
            o.mag = best;
            o.test_statistic = best / o.input_power;
        }
    o.caf_doppler_index = o.doppler_index;
    o.caf_doppler_hz = o.doppler_hz;
    if (cp.half > 0 && crow != 0xffffffffu)
        {
            o.caf_doppler_index = crow;
            o.caf_doppler_hz = doppler_of(ap, crow);
        }
    out[b] = o;
}

int check_iqcaf_handle(const gsdr_acq* a, const char* who)
{
    const int rc = check_single_grid_handle(a, who, "IQ-CAF");
    if (rc != GSDR_OK) return rc;
    GSDR_REQUIRE(a->wipe_mode == GSDR_WIPE_EXACT, GSDR_E_UNSUPPORTED,
        "%s: IQ-CAF runs with the exact carrier only (gsdr_acq_set_wipeoff mode %d)", who, a->wipe_mode);
    return GSDR_OK;
}

// CAF_bins_half of the handle's window and Doppler step (:603); 0 with the filter off.
int32_t caf_half(const gsdr_acq* a, int32_t window_hz)
{
    return window_hz > 0 ? window_hz / (2 * (int32_t)a->conf.doppler_step) : 0;
}

int check_iqcaf_run(const gsdr_acq* a, const char* who)
{
    GSDR_REQUIRE(a->iq.nslots > 0, GSDR_E_STATE, "%s: gsdr_acq_set_iq_caf first", who);
    GSDR_REQUIRE(a->nprn > 0 && a->slots == gsdr_acq::Slots::IqCaf, GSDR_E_STATE, "%s: gsdr_acq_set_iq_codes first", who);
    // gsdr_acq_set_doppler may have changed the step since gsdr_acq_set_iq_caf checked the window
    const int32_t half = caf_half(a, a->iq.window_hz);
    GSDR_REQUIRE(a->iq.window_hz == 0 || (half > 0 && 2ll * half + 1 <= (long long)a->D), GSDR_E_STATE,
        "%s: the CAF window of %d Hz no longer fits the Doppler grid (step %u, %u rows): gsdr_acq_set_iq_caf again", who,
        a->iq.window_hz, a->conf.doppler_step, a->D);
    return check_iqcaf_handle(a, who);
}

// The nitems items at iq (device, fft_size apart) as grids of their own: the input powers, the
// forward spectra and the grid kernel (on a view that carries the run's buffers), the finish
// kernel and the records into iq.d_out, on the handle's stream.
int enqueue_iqcaf(gsdr_acq* a, const void* iq, uint32_t nitems, uint64_t stamp0)
{
    gsdr_acq::IqCaf& q = a->iq;
    hipStream_t s = a->stream;
    StageTimer t(a, s);
    t.begin();
    with_item_type(a->conf.item_type, [&](auto it) {
        hipLaunchKernelGGL((acq_pair_power_kernel<decltype(it)::value>), dim3(nitems), dim3(kPairPowerLanes), 0, s, iq,
            (uint64_t)a->N, a->N, q.d_power);
    });
    GSDR_HIP(hipGetLastError());
    t.end(2);
    AcqView v = view_of(a);
    v.iq_rec = q.d_rec;
    v.iq_rows = q.d_rows;
    v.iq_nslots = q.nslots;
    v.iq_both = q.both;
    v.iq_rows_lds = q.rows_lds;
    AcqOp op{AcqOp::IqCaf, iq, nitems, (uint64_t)a->N, stamp0};
    op.s = s;
    const int rc = dispatch(a, v, op);
    if (rc != GSDR_OK) return rc;
    const uint32_t nsat = v.nprn / q.nslots;
    t.begin();
    hipLaunchKernelGGL(acq_iqcaf_finish_kernel, dim3(nitems * nsat), dim3(64), 0, s,
        (const gsdr_acq_iq_caf_row*)q.d_rec, (const float*)q.d_power, v.prn, q.d_out, params_of(a, v), nsat, q.nslots,
        q.spc, CafParams{caf_half(a, q.window_hz), q.both ? 1u : 0u}, stamp0);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    return GSDR_OK;
}

void free_bufs(gsdr_acq::IqCaf& q)
{
    void* bufs[] = {q.d_in, q.d_rows, q.d_power, q.d_rec, q.d_out};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
}

}  // namespace

void gsdr_acq_impl::iqcaf_free(gsdr_acq* a)
{
    free_bufs(a->iq);
    a->iq = gsdr_acq::IqCaf{};
}

extern "C" {

int gsdr_acq_set_iq_caf(gsdr_acq* a, uint32_t samples_per_code, uint32_t coherent_ms, int both_components,
    int32_t caf_window_hz)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_iq_caf: null handle");
    GSDR_REQUIRE(coherent_ms >= 1 && coherent_ms <= 3, GSDR_E_ARG, "gsdr_acq_set_iq_caf: coherent_ms %u outside [1,3]",
        coherent_ms);
    GSDR_REQUIRE(samples_per_code >= 1 && samples_per_code <= a->N, GSDR_E_ARG,
        "gsdr_acq_set_iq_caf: samples_per_code %u outside [1, fft_size %u]", samples_per_code, a->N);
    std::lock_guard<std::mutex> lk(a->mu);
    int rc = check_iqcaf_handle(a, "gsdr_acq_set_iq_caf");
    if (rc != GSDR_OK) return rc;
    const int32_t half = caf_half(a, caf_window_hz);
    // :605 divides by CAF_bins_half, and the loops of :609-667 stay inside their vectors only
    // while the body's window of 2 half + 1 rows fits the grid
    GSDR_REQUIRE(caf_window_hz <= 0 || half > 0, GSDR_E_ARG,
        "gsdr_acq_set_iq_caf: caf_window_hz %d is below 2 doppler_step (%u): CAF_bins_half would be 0", caf_window_hz,
        a->conf.doppler_step);
    GSDR_REQUIRE(caf_window_hz <= 0 || 2ll * half + 1 <= (long long)a->D, GSDR_E_ARG,
        "gsdr_acq_set_iq_caf: the window of %d rows is wider than the grid's %u", 2 * half + 1, a->D);
    const bool both = both_components != 0;
    const uint32_t nslots = (coherent_ms > 1 ? 2u : 1u) * (both ? 2u : 1u);
    GSDR_REQUIRE(nslots <= a->conf.max_prns, GSDR_E_ARG,
        "gsdr_acq_set_iq_caf: a satellite needs %u code slots, the handle has %u", nslots, a->conf.max_prns);
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipStreamSynchronize(a->stream));
    gsdr_acq::IqCaf fresh{};
    fresh.nslots = nslots;
    fresh.spc = samples_per_code;
    fresh.coherent_ms = coherent_ms;
    fresh.both = both;
    fresh.window_hz = caf_window_hz > 0 ? caf_window_hz : 0;
    fresh.rows_lds = iqcaf_rows_fit_lds(a, nslots);
    const size_t nB = a->conf.max_blocks, nS = a->conf.max_prns / nslots, regions = nB * nS * a->D;
    hipError_t e = hipMalloc(&fresh.d_in, 2 * nS * a->N * sizeof(float2));
    if (e == hipSuccess && !fresh.rows_lds) e = hipMalloc(&fresh.d_rows, regions * nslots * a->N * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_power, nB * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_rec, regions * sizeof(gsdr_acq_iq_caf_row));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_out, nB * nS * sizeof(gsdr_acq_iq_caf_result));
    if (e != hipSuccess)
        {
            free_bufs(fresh);
            gsdr::set_error("gsdr_acq_set_iq_caf: device allocation failed: %s", hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    const gsdr_acq::IqCaf old = a->iq;
    a->iq = fresh;
    rc = dispatch(a, view_of(a), AcqOp{AcqOp::IqCafAttrs});
    if (rc != GSDR_OK)
        {
            free_bufs(fresh);
            a->iq = old;
            return rc;
        }
    gsdr_acq::IqCaf o = old;
    free_bufs(o);
    // slots laid out for other settings are no satellites of these
    if (a->slots == gsdr_acq::Slots::IqCaf) set_slots(a, gsdr_acq::Slots::Plain, 0);
    return GSDR_OK;
}

int gsdr_acq_set_iq_codes(gsdr_acq* a, const float* code_i, const float* code_q, const uint32_t* prn, uint32_t nsat)
{
    GSDR_REQUIRE(a && code_i && prn, GSDR_E_ARG, "gsdr_acq_set_iq_codes: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    gsdr_acq::IqCaf& q = a->iq;
    GSDR_REQUIRE(q.nslots > 0, GSDR_E_STATE, "gsdr_acq_set_iq_codes: gsdr_acq_set_iq_caf first");
    GSDR_REQUIRE((code_q != nullptr) == q.both, GSDR_E_ARG,
        "gsdr_acq_set_iq_codes: code_q must be given with both components and null with one");
    GSDR_REQUIRE(nsat > 0 && (uint64_t)nsat * q.nslots <= a->conf.max_prns, GSDR_E_ARG,
        "gsdr_acq_set_iq_codes: %u satellites need %llu code slots, the handle has %u", nsat,
        (unsigned long long)nsat * q.nslots, a->conf.max_prns);
    gsdr::DeviceGuard g(a->device);
    const size_t row = (size_t)a->N * sizeof(float2);
    float2* d_i = q.d_in;
    float2* d_q = q.d_in + (size_t)(a->conf.max_prns / q.nslots) * a->N;
    std::vector<uint32_t> ids((size_t)nsat * q.nslots);
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = prn[i / q.nslots];
    // ordered after every launch issued so far on the handle's stream
    GSDR_HIP(hipMemcpyAsync(d_i, code_i, nsat * row, hipMemcpyHostToDevice, a->stream));
    if (q.both) GSDR_HIP(hipMemcpyAsync(d_q, code_q, nsat * row, hipMemcpyHostToDevice, a->stream));
    GSDR_HIP(hipMemcpyAsync(a->d_prn, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    // the slots into the staged code rows (consumed == fft_size here)
    hipLaunchKernelGGL(acq_iqcaf_replica_kernel, dim3(nsat), dim3(256), 0, a->stream, (const float2*)d_i,
        (const float2*)d_q, a->d_code_stage, a->N, q.spc, q.coherent_ms > 1 ? 1u : 0u, q.both ? 1u : 0u);
    GSDR_HIP(hipGetLastError());
    const int rc = code_fft(a, 0, nsat * q.nslots);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));  // ids is read until here
    set_slots(a, gsdr_acq::Slots::IqCaf, nsat * q.nslots);
    return GSDR_OK;
}

int gsdr_acq_run_iq_caf(gsdr_acq* a, const void* iq_host, uint32_t nitems, uint64_t stamp0, gsdr_acq_iq_caf_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run_iq_caf: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_iq_caf", nitems, "nitems");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_iqcaf_run(a, "gsdr_acq_run_iq_caf");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)nitems * a->N * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    rc = enqueue_iqcaf(a, a->d_iq, nitems, stamp0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->iq.d_out, (size_t)nitems * (a->nprn / a->iq.nslots) * sizeof(gsdr_acq_iq_caf_result));
}

int gsdr_acq_run_iq_caf_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_iq_caf_result* out)
{
    GSDR_REQUIRE(a && ring && out, GSDR_E_ARG, "gsdr_acq_run_iq_caf_stream: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_iq_caf_stream", nitems, "nitems");
    if (rc == GSDR_OK)
        rc = gsdr::check_ring_consumer("gsdr_acq_run_iq_caf_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_iqcaf_run(a, "gsdr_acq_run_iq_caf_stream");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    rc = with_ring_items(a, ring, first_sample, (uint64_t)nitems * a->N,
        [&](const void* iq) { return enqueue_iqcaf(a, iq, nitems, stamp0); });
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->iq.d_out, (size_t)nitems * (a->nprn / a->iq.nslots) * sizeof(gsdr_acq_iq_caf_result));
}

int gsdr_acq_dump_iq_caf_rows(gsdr_acq* a, const void* iq_host, gsdr_acq_iq_caf_row* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_dump_iq_caf_rows: null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    int rc = check_iqcaf_run(a, "gsdr_acq_dump_iq_caf_rows");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)a->N * gsdr::item_bytes(a->conf.item_type), hipMemcpyHostToDevice,
        a->stream));
    rc = enqueue_iqcaf(a, a->d_iq, 1, 0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->iq.d_rec, (size_t)(a->nprn / a->iq.nslots) * a->D * sizeof(gsdr_acq_iq_caf_row));
}

}  // extern "C"
