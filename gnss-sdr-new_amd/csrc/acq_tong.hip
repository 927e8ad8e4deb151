// Tong acquisition: the launch code and C ABI of gsdr_acq_set_tong, gsdr_acq_tong_reset,
// gsdr_acq_run_tong, gsdr_acq_run_tong_stream and gsdr_acq_dump_tong_grid.  The grid kernel
// template is in acq_tong_kernels.h and is launched through the per-plan dispatch
// (AcqOp::Tong, acq_launch.h) on a view that carries the run's buffers; the kernels that are
// no templates are here.

#include <algorithm>
#include <vector>

#include "acq_handle.h"
#include "acq_power_kernel.h"
#include "gsdr_stream_internal.h"

using namespace gsdr_acq_impl;

namespace
{

// set_state(1) (:188-210) of slots [first, first + n): the counts back to their start, the
// sequence running.  dwell_count == 0 also tells the grid kernel to start the slot's rows from
// zero, which is the reference's pass over d_grid_data.
__global__ void __launch_bounds__(64) acq_tong_reset_kernel(TongSlot* __restrict__ slots, uint32_t first, uint32_t n,
    uint32_t init)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) slots[first + i] = TongSlot{0u, init, GSDR_TONG_RUNNING, 0u};
}

// The items' scales 1 / (fn fn P_k), fn = float(N) float(N), all in float (:268, :312-314).
__global__ void __launch_bounds__(64) acq_tong_scale_kernel(const float* __restrict__ power, float* __restrict__ scale,
    uint32_t nitems, uint32_t n)
{
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nitems) return;
    const float fn = gsdr::mul_rn((float)n, (float)n);
    scale[k] = 1.0f / gsdr::mul_rn(gsdr::mul_rn(fn, fn), power[k]);
}

// ---------------------------------------------------------------- K_tong_update
// One wave per slot, the call's items in order.  Per item: the winner among the D row maxima
// of the accumulated grid -- the first row holding the maximum (d_mag < magt with rows
// ascending, :325) and that row's first index (:320) -- then the counter (:349-372): up when
// mag > threshold * dwell_count, positive when it equals tong_max_val; else down, negative at
// zero; then negative whenever dwell_count has reached tong_max_dwells, a positive of that
// same dwell included.  The slot's state goes back to device memory once, after the last item;
// items after the terminal one get GSDR_TONG_PAST_END records and leave it alone.
__global__ void __launch_bounds__(64) acq_tong_update_kernel(const RowStat* __restrict__ stats,
    const float* __restrict__ power, TongSlot* __restrict__ slots, const uint32_t* __restrict__ prn,
    gsdr_acq_tong_result* __restrict__ out, AcqParams ap, uint32_t nitems, uint32_t tong_max, uint32_t max_dwells,
    uint64_t stamp0)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    TongSlot sl = slots[p];
    const uint32_t spc = (uint32_t)ap.samples_per_code;
    for (uint32_t k = 0; k < nitems; ++k)
        {
            gsdr_acq_tong_result r{};
            r.prn = prn[p];
            r.samplestamp = stamp0 + (uint64_t)k * ap.N;
            r.input_power = power[k];
            if (sl.state != GSDR_TONG_RUNNING)
                {
                    r.dwell_count = sl.dwell_count;
                    r.tong_count = sl.tong_count;
                    r.state = GSDR_TONG_PAST_END;
                    if (lane == 0) out[(size_t)k * ap.P + p] = r;
                    continue;
                }
            float best = -1.0f;
            uint32_t brow = 0xffffffffu, bidx = 0;
            const RowStat* st = stats + ((size_t)k * ap.P + p) * ap.D;
            for (uint32_t d = lane; d < ap.D; d += 64)
                {
                    const RowStat s = st[d];
                    if (stat_better(s.max, d, best, brow))
                        {
                            best = s.max;
                            brow = d;
                            bidx = s.idx;
                        }
                }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                {
                    const float om = __shfl_xor(best, off);
                    const uint32_t orow = __shfl_xor(brow, off), oidx = __shfl_xor(bidx, off);
                    if (stat_better(om, orow, best, brow))
                        {
                            best = om;
                            brow = orow;
                            bidx = oidx;
                        }
                }
            sl.dwell_count += 1;
            // a grid of zeros leaves the synchro fields as the reset wrote them (d_mag < magt, :325)
            if (best > 0.0f)
                {
                    r.doppler_index = brow;
                    r.indext = bidx;
                    r.doppler_hz = doppler_of(ap, brow);
                    r.acq_delay_samples = (double)(spc > 0 ? bidx % spc : bidx);
                    r.mag = best;
                }
            if (r.mag > gsdr::mul_rn(ap.threshold, (float)sl.dwell_count))
                {
                    sl.tong_count += 1;
                    if (sl.tong_count == tong_max) sl.state = GSDR_TONG_POSITIVE;
                }
            else
                {
                    sl.tong_count -= 1;
                    if (sl.tong_count == 0) sl.state = GSDR_TONG_NEGATIVE;
                }
            if (sl.dwell_count >= max_dwells) sl.state = GSDR_TONG_NEGATIVE;
            r.dwell_count = sl.dwell_count;
            r.tong_count = sl.tong_count;
            r.state = sl.state;
            if (lane == 0) out[(size_t)k * ap.P + p] = r;
        }
    if (lane == 0) slots[p] = sl;
}

// What a Tong call needs of the handle; `who` names the call in the message.
int check_tong_handle(const gsdr_acq* a, const char* who)
{
    const int rc = check_single_grid_handle(a, who, "Tong");
    if (rc != GSDR_OK) return rc;
    GSDR_REQUIRE(a->variant < 20, GSDR_E_UNSUPPORTED,
        "%s: fft_size %u runs on a four-step plan; the walking grid kernel needs a one-launch LDS plan", who, a->N);
    GSDR_REQUIRE(a->wipe_mode == GSDR_WIPE_EXACT, GSDR_E_UNSUPPORTED,
        "%s: Tong runs with the exact carrier only (gsdr_acq_set_wipeoff mode %d)", who, a->wipe_mode);
    return GSDR_OK;
}

int check_tong_run(const gsdr_acq* a, const char* who)
{
    GSDR_REQUIRE(a->tong.max > 0, GSDR_E_STATE, "%s: gsdr_acq_set_tong first", who);
    GSDR_REQUIRE(a->nprn > 0 && a->slots == gsdr_acq::Slots::Plain, GSDR_E_STATE, "%s: gsdr_acq_set_local_codes first",
        who);
    GSDR_REQUIRE(a->wipe_mode == GSDR_WIPE_EXACT, GSDR_E_UNSUPPORTED,
        "%s: Tong runs with the exact carrier only (gsdr_acq_set_wipeoff mode %d)", who, a->wipe_mode);
    return GSDR_OK;
}

int enqueue_reset(gsdr_acq* a, uint32_t first, uint32_t n)
{
    hipLaunchKernelGGL(acq_tong_reset_kernel, dim3((n + 63) / 64), dim3(64), 0, a->stream, a->tong.d_slots, first, n,
        a->tong.init);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

// The nitems items at iq (device, fft_size apart) continue every active slot's sequence: the
// input powers and scales, the forward spectra and the grid kernel (on a view that carries the
// run's buffers), the counter kernel and the records into tong.d_out, on the handle's stream.
int enqueue_tong(gsdr_acq* a, const void* iq, uint32_t nitems, uint64_t stamp0)
{
    gsdr_acq::Tong& tg = a->tong;
    hipStream_t s = a->stream;
    StageTimer t(a, s);
    t.begin();
    with_item_type(a->conf.item_type, [&](auto it) {
        hipLaunchKernelGGL((acq_pair_power_kernel<decltype(it)::value>), dim3(nitems), dim3(kPairPowerLanes), 0, s, iq,
            (uint64_t)a->N, a->N, tg.d_power);
    });
    GSDR_HIP(hipGetLastError());
    hipLaunchKernelGGL(acq_tong_scale_kernel, dim3((nitems + 63) / 64), dim3(64), 0, s, (const float*)tg.d_power,
        tg.d_scale, nitems, a->N);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    AcqView v = view_of(a);
    v.tong_grid = tg.d_grid;
    v.tong_scale = tg.d_scale;
    v.tong_slots = tg.d_slots;
    v.tong_stats = tg.d_stats;
    v.tong_row_lds = tg.row_lds;
    AcqOp op{AcqOp::Tong, iq, nitems, (uint64_t)a->N, stamp0};
    op.s = s;
    const int rc = dispatch(a, v, op);
    if (rc != GSDR_OK) return rc;
    t.begin();
    hipLaunchKernelGGL(acq_tong_update_kernel, dim3(v.nprn), dim3(64), 0, s, (const RowStat*)tg.d_stats,
        (const float*)tg.d_power, tg.d_slots, v.prn, tg.d_out, params_of(a, v), nitems, tg.max, tg.max_dwells, stamp0);
    GSDR_HIP(hipGetLastError());
    t.end(2);
    return GSDR_OK;
}

}  // namespace

void gsdr_acq_impl::tong_free(gsdr_acq* a)
{
    gsdr_acq::Tong& tg = a->tong;
    void* bufs[] = {tg.d_grid, tg.d_slots, tg.d_power, tg.d_scale, tg.d_stats, tg.d_out};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    tg = gsdr_acq::Tong{};
}

extern "C" {

int gsdr_acq_set_tong(gsdr_acq* a, uint32_t tong_init_val, uint32_t tong_max_val, uint32_t tong_max_dwells)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_set_tong: null handle");
    // the reference's unsigned d_tong_count wraps below zero from init 0, and a count that
    // starts at or above tong_max_val never meets the '==' of :355
    GSDR_REQUIRE(tong_init_val >= 1 && tong_init_val < tong_max_val, GSDR_E_ARG,
        "gsdr_acq_set_tong: need 1 <= tong_init_val (%u) < tong_max_val (%u)", tong_init_val, tong_max_val);
    GSDR_REQUIRE(tong_max_dwells >= 1, GSDR_E_ARG, "gsdr_acq_set_tong: tong_max_dwells must be >= 1");
    std::lock_guard<std::mutex> lk(a->mu);
    int rc = check_tong_handle(a, "gsdr_acq_set_tong");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipStreamSynchronize(a->stream));
    gsdr_acq::Tong fresh{};
    const size_t nB = a->conf.max_blocks, nP = a->conf.max_prns, rows = nP * a->D;
    hipError_t e = hipMalloc(&fresh.d_grid, rows * a->N * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_slots, nP * sizeof(TongSlot));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_power, nB * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_scale, nB * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_stats, nB * rows * sizeof(RowStat));
    if (e == hipSuccess) e = hipMalloc(&fresh.d_out, nB * nP * sizeof(gsdr_acq_tong_result));
    if (e != hipSuccess)
        {
            void* bufs[] = {fresh.d_grid, fresh.d_slots, fresh.d_power, fresh.d_scale, fresh.d_stats, fresh.d_out};
            for (void* p : bufs)
                if (p) (void)hipFree(p);
            gsdr::set_error("gsdr_acq_set_tong: device allocation failed: %s", hipGetErrorString(e));
            return GSDR_E_ALLOC;
        }
    tong_free(a);
    a->tong = fresh;
    a->tong.init = tong_init_val;
    a->tong.max = tong_max_val;
    a->tong.max_dwells = tong_max_dwells;
    a->tong.row_lds = tong_row_fits_lds(a);
    rc = enqueue_reset(a, 0, (uint32_t)nP);
    if (rc == GSDR_OK && hipStreamSynchronize(a->stream) != hipSuccess) rc = GSDR_E_DEVICE;
    if (rc != GSDR_OK) tong_free(a);
    return rc;
}

int gsdr_acq_tong_reset(gsdr_acq* a, const uint32_t* slots, uint32_t nslots)
{
    GSDR_REQUIRE(a, GSDR_E_ARG, "gsdr_acq_tong_reset: null handle");
    std::lock_guard<std::mutex> lk(a->mu);
    GSDR_REQUIRE(a->tong.max > 0, GSDR_E_STATE, "gsdr_acq_tong_reset: gsdr_acq_set_tong first");
    gsdr::DeviceGuard g(a->device);
    if (!slots) return enqueue_reset(a, 0, a->conf.max_prns);
    for (uint32_t i = 0; i < nslots; ++i)
        GSDR_REQUIRE(slots[i] < a->conf.max_prns, GSDR_E_ARG, "gsdr_acq_tong_reset: slot %u outside [0,%u)", slots[i],
            a->conf.max_prns);
    // behind the work enqueued so far on the handle's stream, as the runs are
    for (uint32_t i = 0; i < nslots; ++i)
        {
            const int rc = enqueue_reset(a, slots[i], 1);
            if (rc != GSDR_OK) return rc;
        }
    return GSDR_OK;
}

int gsdr_acq_run_tong(gsdr_acq* a, const void* iq_host, uint32_t nitems, uint64_t stamp0, gsdr_acq_tong_result* out)
{
    GSDR_REQUIRE(a && iq_host && out, GSDR_E_ARG, "gsdr_acq_run_tong: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_tong", nitems, "nitems");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_tong_run(a, "gsdr_acq_run_tong");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    GSDR_HIP(hipMemcpyAsync(a->d_iq, iq_host, (size_t)nitems * a->N * gsdr::item_bytes(a->conf.item_type),
        hipMemcpyHostToDevice, a->stream));
    rc = enqueue_tong(a, a->d_iq, nitems, stamp0);
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->tong.d_out, (size_t)nitems * a->nprn * sizeof(gsdr_acq_tong_result));
}

int gsdr_acq_run_tong_stream(gsdr_acq* a, gsdr_stream* ring, uint64_t first_sample, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_tong_result* out)
{
    GSDR_REQUIRE(a && ring && out, GSDR_E_ARG, "gsdr_acq_run_tong_stream: null argument");
    int rc = check_block_count(a, "gsdr_acq_run_tong_stream", nitems, "nitems");
    if (rc == GSDR_OK)
        rc = gsdr::check_ring_consumer("gsdr_acq_run_tong_stream", ring, a->conf.item_type, a->device, "acquisition");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    rc = check_tong_run(a, "gsdr_acq_run_tong_stream");
    if (rc != GSDR_OK) return rc;
    gsdr::DeviceGuard g(a->device);
    rc = with_ring_items(a, ring, first_sample, (uint64_t)nitems * a->N,
        [&](const void* iq) { return enqueue_tong(a, iq, nitems, stamp0); });
    if (rc != GSDR_OK) return rc;
    return read_back(a, out, a->tong.d_out, (size_t)nitems * a->nprn * sizeof(gsdr_acq_tong_result));
}

int gsdr_acq_dump_tong_grid(gsdr_acq* a, uint32_t prn_slot, float* grid_host)
{
    GSDR_REQUIRE(a && grid_host, GSDR_E_ARG, "gsdr_acq_dump_tong_grid: null argument");
    GSDR_REQUIRE(prn_slot < a->conf.max_prns, GSDR_E_ARG, "gsdr_acq_dump_tong_grid: prn_slot %u outside [0,%u)",
        prn_slot, a->conf.max_prns);
    std::lock_guard<std::mutex> lk(a->mu);
    GSDR_REQUIRE(a->tong.max > 0, GSDR_E_STATE, "gsdr_acq_dump_tong_grid: gsdr_acq_set_tong first");
    gsdr::DeviceGuard g(a->device);
    const size_t n = (size_t)a->D * a->N;
    TongSlot sl{};
    GSDR_HIP(hipMemcpyAsync(&sl, a->tong.d_slots + prn_slot, sizeof(sl), hipMemcpyDeviceToHost, a->stream));
    const int rc = read_back(a, grid_host, a->tong.d_grid + (size_t)prn_slot * n, n * sizeof(float));
    if (rc != GSDR_OK) return rc;
    // no item since the reset: the rows are what the slot's next item starts from
    if (sl.dwell_count == 0) std::fill(grid_host, grid_host + n, 0.0f);
    return GSDR_OK;
}

}  // extern "C"
