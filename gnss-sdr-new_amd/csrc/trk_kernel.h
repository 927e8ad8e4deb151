// Device-resident DLL/PLL tracking loop for MI355X (gfx950).
//
// Restates dll_pll_veml_tracking (src/algorithms/tracking/gnuradio_blocks/
// dll_pll_veml_tracking.cc) for GPS L1 C/A as one kernel that keeps every
// channel's loop state on the device: one workgroup per channel iterates over
// its general_work calls ("epochs") without returning to the host --
//
//   correlation  (do_correlation_step, :1064-1089) -- 256 lanes, fused carrier
//                wipe-off + code resampler + E/P/L dot products, replica in LDS;
//   loop update  (lane 0)  save results / cn0_and_tracking_lock_status (:970-1056)
//                / run_dll_pll (:1092-1179) / update_tracking_vars (:1216-1287)
//                / bit synchronisation (acquire_secondary, :923-967) and the
//                state machine of general_work (:1784-2152, states 2 and 4).
//
// The tracking loop is sequential in time per channel (each epoch's NCO comes
// from the previous epoch's discriminators), so the parallel axes are the
// samples of one correlation and the channels; the per-epoch host round trip of
// the reference (one general_work call per code period) becomes a loop inside
// one launch.
//
// Types follow the reference members (dll_pll_veml_tracking.h:117-209): float
// where it uses float, double where it uses double, so the device loop tracks
// the CPU restatement (oracle/trk_oracle.c) to fp rounding.
#pragma once
#include "trk_correlate.h"
#include "trk_kf_step.h"
#include "trk_loop.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

namespace
{
using namespace gsdr::trk;

// The loop state make_prep reads (wave 0 -> wave 1 after the locked branch): wave 1 plans
// the next call while wave 0 takes the lock test and writes the record
struct PlanIn
{
    double carrier_phase_step_rad, carrier_phase_rate_step_rad, rem_code_phase_chips, code_phase_step_chips,
        code_phase_rate_step_chips;
    uint64_t next_sample;
    float rem_carr_phase_rad;
    int32_t state, narrow;
};

// One call's NCO and read plan from the loop state (lane-uniform): computed by
// wave 0 at the end of the previous call's update, where the state is still in
// registers (launch start: by lane 0 from the LDS copy).
__device__ __forceinline__ Prep make_prep(const TrkConst& c, const TrkHot& t, bool go_epoch, uint64_t iq_first,
    uint64_t iq_items, int vl, int K, int L, bool use_window, bool streamed, int stream_chunk, int64_t win_base,
    int64_t pf_first)
{
    Prep p{};
    const int64_t off = (int64_t)(t.next_sample - iq_first);
    p.go = go_epoch && t.state >= 2 && t.state <= 4 && t.next_sample >= iq_first &&
           (uint64_t)off + (uint64_t)vl <= iq_items;
    p.off = off;
    p.narrow = t.narrow;
    p.woff = -1;
    if (use_window && win_base != INT64_MIN && off >= win_base && off - win_base + vl <= kWinCore + kHalo)
        p.woff = (int32_t)(off - win_base);
    p.pf_ok = streamed && pf_first != INT64_MIN && off >= pf_first &&
              off + min(vl, stream_chunk) <= pf_first + stream_chunk + kHalo;
    if (p.go)
        {
            // do_correlation_step's float arguments (:1069-1075); the
            // reference's phasors (cos r, -sin r) and exp(-j step)
            // (cpu_multicorrelator_real_codes.cc:114-123) as angles
            const float rem_carr = t.rem_carr_phase_rad;
            const float carr_step = (float)t.carrier_phase_step_rad;
            p.rem_code = (float)t.rem_code_phase_chips * (float)c.code_samples_per_chip;
            p.code_step = (float)t.code_phase_step_chips * (float)c.code_samples_per_chip;
            p.psi0 = -(double)rem_carr;
            p.theta = -(double)carr_step;
            // index range of the call (monotone in n for step > 0)
            // static tap indices throughout: a run-time index into p
            // (hdshift) sent the whole Prep through scratch
            float smin = 1e30f, smax = -1e30f;
#pragma unroll
            for (int k = 0; k < kMaxTrkTaps; ++k)
                {
                    if (k < K)
                        {
                            const float sr =
                                gsdr::sub_rn(t.narrow ? c.shifts_narrow[k] : c.shifts[k], p.rem_code);
                            smin = fminf(smin, sr);
                            smax = fmaxf(smax, sr);
                        }
                }
            const float lo = floorf(smin);
            const float hi = floorf(gsdr::add_rn(gsdr::mul_rn(p.code_step, (float)(vl - 1)), smax));
            const float Lf = (float)L;
            const bool mono = p.code_step >= 0.0f;
            p.wrap = (mono && lo >= -(float)kCodeMargin && hi < Lf + (float)kCodeMargin)
                         ? 2
                         : ((mono && lo >= -Lf && hi < 2.0f * Lf) ? 1 : 0);
            if (c.high_dyn)
                {
                    p.hd = 1;
                    p.theta_rate = -(double)(float)t.carrier_phase_rate_step_rad;
                    p.code_rate = (float)t.code_phase_rate_step_chips * (float)c.code_samples_per_chip;
                    unsigned int shs = 0;
                    p.hdshift[0] = 0;
#pragma unroll
                    for (int k = 1; k < kMaxTrkTaps; ++k)
                        {
                            if (k < K)
                                {
                                    const float* sk = t.narrow ? c.shifts_narrow : c.shifts;
                                    shs += (int)roundf((sk[k] - sk[k - 1]) / p.code_step);
                                    p.hdshift[k] = (int)shs;
                                }
                        }
                }
            const double w = p.theta * (double)kTrkThreads;
            float sn, cs;
            sincosf((float)fma(-rint(w * 0.15915494309189533576888376337251), 6.283185307179586476925286766559, w),
                &sn, &cs);
            p.wstep = make_float2(cs, sn);
        }
    return p;
}

// grid = channels; one kTrkThreads-lane workgroup per channel.  Wave 0 holds the
// mutable loop state in registers for the whole launch (uniform across its
// lanes); the configuration comes through scalar loads; the histories indexed at
// run time (CN0 buffer, DLL filter), the replica and the next call's input window
// sit in LDS.  While wave 0 runs the loop update of call e, every lane fetches
// the samples call e+1 will most likely read (the consumed count is one code
// period +-1 sample), so the update hides the HBM latency.
// PACK: every channel of the launch tracks a pilot on the compact replica (see
// correlate_chunk); the handle launches it instead when its replicas qualify.
// KF: the Kalman loop (gsdr_trk_set_kf) in the DLL/PLL loop's place: wave 1 runs the
// discriminators, the prediction and P- H^T as soon as the accumulators are known and, in
// state 4 only, waits for wave 2's C/N0 where d_R enters the innovation covariance; wave 0
// takes x for the NCO commands while wave 1 finishes P; wave 3 has no code loop to run.
template <int IT, bool PACK = false, bool KF = false>
__global__ void __launch_bounds__(kTrkThreads) trk_kernel(const TrkConst* __restrict__ consts,
    TrkChan* __restrict__ chans, const float* const* __restrict__ codes, const float* const* __restrict__ data_codes,
    const void* __restrict__ iq, uint64_t iq_first, uint64_t iq_items, uint32_t max_epochs, gsdr_trk_epoch* __restrict__ out,
    uint32_t* __restrict__ nout, int code_pad, int data_pad, uint64_t* __restrict__ timing, int timing_wall, int stream_chunk,
    int sbuf_bytes)
{
    // LDS: [replica | data replica (pilot tracking) | next call's input window];
    // PACK: [compact replica (pilot and data chips) | next call's input window], data_pad = 0
    extern __shared__ float s_dyn[];
    // replicas with kCodeMargin wrapped samples on each side: s_code[-M .. L+M)
    float* s_code = s_dyn + kCodeMargin;
    float* s_data = s_dyn + code_pad + kCodeMargin;
    float2* s_win = reinterpret_cast<float2*>(s_dyn + code_pad + data_pad);
    char* s_sb = reinterpret_cast<char*>(s_dyn + code_pad + data_pad);  // streamed calls: two chunk buffers
    __shared__ LoopFilter s_lfs[2];  // code loop filter: current slot and wave 3's speculative one
    __shared__ int s_lfi;
    __shared__ DllPllSpec s_spec;
    __shared__ int s_spec_e;
    __shared__ DllSpec s_dspec;
    __shared__ int s_dspec_e;
    __shared__ float2 s_pbuf[kMaxCn0];
    __shared__ __attribute__((aligned(16))) float s_cn[3][kMaxCn0];  // cn0_and_lock's per-element terms
    __shared__ __attribute__((aligned(16))) float s_evm_buf[2 * kMaxCn0];  // evm_of's (wave 1)
    __shared__ double s_evm;
    __shared__ int s_evm_e;
    __shared__ Cn0Spec s_cn0;  // wave 2's lock test of the call (cn0_and_lock)
    __shared__ int s_cn0_e;
    __shared__ PlanIn s_plan;  // wave 0's loop state for wave 1's next-call plan
    __shared__ uint64_t s_w2t[3];  // GSDR_TRK_TIMING: wave 2's lock test start / end, wave 1's EVM end
    __shared__ int s_plan_e, s_prep_e;
    __shared__ int s_state;
    __shared__ Prep prep;
    __shared__ float2 s_red[kTrkThreads / 64][kMaxTrkTaps + 1];
    // the loop state lives in LDS between calls and in wave 0's registers only
    // during the loop update, so the correlation keeps its registers for loads
    // in flight (with the state resident for the whole launch the kernel sat at
    // 256 VGPRs and the compiler serialised the sample loads)
    __shared__ TrkHot s_t;
    __shared__ int s_overrun;  // the channel fell behind the input (one loss-of-lock record)
    const int ch = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TrkConst& c = consts[ch];
    TrkChan* gc = chans + ch;
    if constexpr (KF)
        {
            KfShared* const ks = kf_shared<true>();
            if (tid < 16) ks->slot[0].P[tid] = gc->kf.P[tid];
            if (tid < 16) ks->q[tid] = gc->kf.Q[tid];
            if (tid < 4) ks->slot[0].x[tid] = gc->kf.x[tid];
            if (tid < 2) ks->r[tid] = gc->kf.R[tid];
            if (tid == 0) ks->cur = 0;
        }
    // The tracking loop is a latency chain that shares its CUs with the
    // acquisition grid running on another queue: raise the issue priority.
    __builtin_amdgcn_s_setprio(3);
    if (tid == 0)
        {
            s_t = gc->h;
            s_lfs[0] = gc->code_filter;
            s_lfi = 0;
            s_spec_e = -1;
            s_dspec_e = -1;
            s_evm_e = -1;
            s_cn0_e = -1;
            s_plan_e = -1;
            s_prep_e = -1;
            s_state = s_t.state;
            s_overrun = 0;
        }
    if (tid < kMaxCn0) s_pbuf[tid] = gc->prompt_buffer[tid];
    __syncthreads();
    if (s_state < 2 || s_state > 4)
        {
            if (tid == 0) nout[ch] = 0;
            return;
        }
    const int K = c.n_taps;
    const int L = c.code_samples;
    const int vl = c.vector_length;
    // calls of at most kWinCore samples: the next call's window staged by waves 3.. through
    // registers (the streamed path's LDS-DMA prefetch for them measured 181 -> 213 ticks of
    // correlation per C2 call, profiles/r06r)
    const bool use_window = vl <= kWinCore;
    const bool streamed = !use_window && stream_chunk > 0;
    const bool data = c.track_pilot != 0;
    {
        const float* cd = codes[ch];
        if constexpr (PACK)
            {
                const float* dd = data_codes[ch];
                for (int i = tid - kCodeMargin; i < L + kCodeMargin; i += kTrkThreads)
                    {
                        const int m = ((i % L) + L) % L;
                        const uint32_t lo = __builtin_bit_cast(unsigned short, (_Float16)cd[m]);
                        const uint32_t hi = __builtin_bit_cast(unsigned short, (_Float16)dd[m]);
                        s_code[i] = __uint_as_float(lo | (hi << 16));
                    }
            }
        else
            {
                for (int i = tid - kCodeMargin; i < L + kCodeMargin; i += kTrkThreads) s_code[i] = cd[((i % L) + L) % L];
                if (data)
                    {
                        const float* dd = data_codes[ch];
                        for (int i = tid - kCodeMargin; i < L + kCodeMargin; i += kTrkThreads)
                            s_data[i] = dd[((i % L) + L) % L];
                    }
            }
    }
    int64_t win_base = INT64_MIN;  // absolute-index base of the staged window (uniform)
    int lfi0 = 0;                  // wave 0: the current code loop filter slot (s_lfi)
    int64_t pf_first = INT64_MIN;  // streamed calls: first sample of the prefetched chunk 0 (uniform)
    uintptr_t pf_start[2] = {0, 0};  // and the byte addresses chunks 0 / 1's LDS buffers start at (0: not fetched)
    uint32_t e = 0;
    for (;; ++e)
        {
            uint64_t tm0 = 0, tm1 = 0, tm2 = 0, swait = 0;
            if (timing && tid == 0) tm0 = wall_clock64();
            if (tid == 0 && e == 0)
                {
                    const TrkHot& t = s_t;
                    if (e == 0 && t.state >= 2 && t.state <= 4 && t.next_sample < iq_first && max_epochs > 0)
                        {
                            // the channel's next call starts before the oldest item the
                            // caller provides (a ring that moved past a stalled channel):
                            // it can never continue, so report it as a loss of lock
                            // (event 3, the Channel FSM re-acquires) instead of stalling
                            gsdr_trk_epoch r{};
                            r.sample_counter = t.next_sample;
                            r.state = t.state;
                            r.flags = GSDR_TRK_F_LOSS_OF_LOCK | GSDR_TRK_F_OVERRUN;
                            r.carrier_doppler_hz = t.carrier_doppler_hz;
                            r.code_freq_chips = t.code_freq_chips;
                            r.cn0_db_hz = t.cn0_db_hz;
                            out[(size_t)ch * max_epochs] = r;
                            clear_tracking_vars(s_t);
                            s_t.state = 0;
                            s_overrun = 1;
                        }
                    prep = make_prep(c, t, e < max_epochs, iq_first, iq_items, vl, K, L, use_window, streamed,
                        stream_chunk, win_base, pf_first);
                }
            __syncthreads();
            if (!prep.go) break;
            if (timing && tid == 0) tm1 = wall_clock64();
            // ---- correlation: lane-interleaved samples, fp64 phasor anchor + fp32 steps
            // the plan read from LDS where it is used (a register copy lived across the
            // whole correlation and the allocator spilled it); the offset is read once,
            // before wave 0 can write the next plan
            const Prep& p = prep;
            const int64_t p_off = p.off;
            float2 acc[kMaxTrkTaps + 1];
#pragma unroll
            for (int k = 0; k <= kMaxTrkTaps; ++k) acc[k] = make_float2(0.f, 0.f);
            float2 ph;
            {
                const double phi = p.psi0 + (double)tid * p.theta;
                const float a = (float)fma(-rint(phi * 0.15915494309189533576888376337251), 6.283185307179586476925286766559, phi);
                float sn, cs;
                sincosf(a, &sn, &cs);
                ph = make_float2(cs, sn);
            }
            float sh_rem[kMaxTrkTaps];
#pragma unroll
            for (int k = 0; k < kMaxTrkTaps; ++k)
                sh_rem[k] = gsdr::sub_rn(p.narrow ? c.shifts_narrow[k] : c.shifts[k], p.rem_code);
            if constexpr (PACK)
                {
                    // pilot tracking without high_dyn (the host launches this kernel for nothing else)
                    const bool sw = timing && tid == 0;
                    if (streamed && K <= 3)
                        correlate_call_stream<IT, 3, true, true>(iq, iq_items, s_sb, sbuf_bytes, stream_chunk, p.pf_ok, pf_start,
                            s_code, s_data, p, vl, L, sh_rem, ph, acc, sw, swait);
                    else if (streamed)
                        correlate_call_stream<IT, kMaxTrkTaps, true, true>(iq, iq_items, s_sb, sbuf_bytes, stream_chunk, p.pf_ok,
                            pf_start, s_code, s_data, p, vl, L, sh_rem, ph, acc, sw, swait);
                    else if (K <= 3)
                        correlate_call<IT, 3, true, true>(iq, s_win, s_code, s_data, p, vl, L, sh_rem, ph, acc);
                    else
                        correlate_call<IT, kMaxTrkTaps, true, true>(iq, s_win, s_code, s_data, p, vl, L, sh_rem, ph, acc);
                }
            else if (p.hd)
                {
                    const float* sk = p.narrow ? c.shifts_narrow : c.shifts;
                    correlate_call_hd<IT>(iq, s_win, s_code, s_data, p, vl, L, K, data, sk[0], sk[c.iP], acc);
                }
            else if (streamed)
                {
                    const bool sw = timing && tid == 0;
                    if (K <= 3)
                        correlate_call_stream<IT, 3, false>(iq, iq_items, s_sb, sbuf_bytes, stream_chunk, p.pf_ok, pf_start,
                            s_code, s_data, p, vl, L, sh_rem, ph, acc, sw, swait);
                    else if (!data)
                        correlate_call_stream<IT, kMaxTrkTaps, false>(iq, iq_items, s_sb, sbuf_bytes, stream_chunk, p.pf_ok,
                            pf_start, s_code, s_data, p, vl, L, sh_rem, ph, acc, sw, swait);
                    else
                        correlate_call_stream<IT, kMaxTrkTaps, true>(iq, iq_items, s_sb, sbuf_bytes, stream_chunk, p.pf_ok,
                            pf_start, s_code, s_data, p, vl, L, sh_rem, ph, acc, sw, swait);
                }
            else if (K <= 3)
                correlate_call<IT, 3, false>(iq, s_win, s_code, s_data, p, vl, L, sh_rem, ph, acc);
            else if (!data)
                correlate_call<IT, kMaxTrkTaps, false>(iq, s_win, s_code, s_data, p, vl, L, sh_rem, ph, acc);
            else
                correlate_call<IT, kMaxTrkTaps, true>(iq, s_win, s_code, s_data, p, vl, L, sh_rem, ph, acc);
#pragma unroll
            for (int k = 0; k <= kMaxTrkTaps; ++k)
                {
                    if (k < K || (k == kMaxTrkTaps && data))
                        {
                            // wave sums by DPP (the total in lane 63)
                            acc[k].x = gsdr::wave_sum_lane63(acc[k].x);
                            acc[k].y = gsdr::wave_sum_lane63(acc[k].y);
                        }
                }
            if (lane == 63)
                {
#pragma unroll
                    for (int k = 0; k <= kMaxTrkTaps; ++k) s_red[wave][k] = acc[k];
                }
            __syncthreads();  // partials visible; every read of the LDS window done
            if (timing && tid == 0) tm2 = wall_clock64();
            // lane k sums tap k over the waves in wave order (one batch of LDS reads
            // instead of a serial read per partial), then every lane takes the totals
            // by readlane; E/P/L are the same sums
            auto tap_totals = [&](float2 (&taps)[kMaxTrkTaps + 1], float2 (&epl)[3]) {
                float2 mine = make_float2(0.f, 0.f);
                if (lane <= kMaxTrkTaps)
                    {
                        float2 v[kTrkThreads / 64];
#pragma unroll
                        for (int w = 0; w < kTrkThreads / 64; ++w) v[w] = s_red[w][lane];
#pragma unroll
                        for (int w = 0; w < kTrkThreads / 64; ++w)
                            {
                                mine.x += v[w].x;
                                mine.y += v[w].y;
                            }
                    }
#pragma unroll
                for (int k = 0; k <= kMaxTrkTaps; ++k)
                    taps[k] = (k < K || (k == kMaxTrkTaps && data)) ? make_float2(lane_f(mine.x, k), lane_f(mine.y, k))
                                                                   : make_float2(0.f, 0.f);
                const int ix[3] = {c.iE, c.iP, c.iL};
#pragma unroll
                for (int q = 0; q < 3; ++q) epl[q] = make_float2(lane_f(mine.x, ix[q]), lane_f(mine.y, ix[q]));
            };
            if (!KF && wave == 3)
                {
                    // this call's code loop (DLL discriminator and filter) on a copy of
                    // the state, into the code loop filter slot that is not current; wave
                    // 1 runs the carrier loop at the same time (take_dll_pll joins them).
                    // Before this wave's share of the window staging / prefetch, which
                    // only has to land before the next call
                    TrkHot t3 = s_t;
                    if (t3.state == 2 || t3.state == 4)
                        {
                            float2 taps[kMaxTrkTaps + 1], epl[3];
                            tap_totals(taps, epl);
                            if (t3.state == 2)
                                {
                                    if (c.veml)
                                        {
                                            t3.VE_accu = taps[0];
                                            t3.VL_accu = taps[4];
                                        }
                                    t3.E_accu = epl[0];
                                    t3.P_accu = epl[1];
                                    t3.L_accu = epl[2];
                                    t3.spc = c.early_late_space_chips;
                                }
                            else
                                save_correlation_results(c, t3, taps, epl);
                            // the filter in registers, written to the other slot after
                            const int cur = s_lfi;
                            LfReg lf3 = lf_load(s_lfs[cur]);
                            const double base = run_dll(c, t3, lf3);
                            if (lane == 0)
                                {
                                    LoopFilter& d = s_lfs[cur ^ 1];
                                    d = s_lfs[cur];
                                    d.inputs[0] = lf3.i0;
                                    d.inputs[1] = lf3.i1;
                                    d.inputs[2] = lf3.i2;
                                    d.inputs[3] = lf3.i3;
                                    d.outputs[0] = lf3.o0;
                                    d.outputs[1] = lf3.o1;
                                    d.outputs[2] = lf3.o2;
                                    d.outputs[3] = lf3.o3;
                                    d.idx = lf3.idx;
                                    DllSpec r;
                                    r.code_freq_base = base;
                                    r.log_err2 = t3.log_err[2];
                                    r.log_err3 = t3.log_err[3];
                                    s_dspec = r;
                                    __hip_atomic_store(&s_dspec_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                        }
                }
            // ---- stage the window the next call most likely reads, [off + vl - kHalo/2,
            // +kWinCore+kHalo), into LDS: waves 3.. only (wave 3 after its code loop),
            // while wave 0 runs the loop update, wave 1 the carrier loop and the EVM and
            // wave 2 the lock test (every read of the current window is done), so wave 0
            // issues no global loads that a vmcnt wait inside its update would wait for
            const int64_t nb = p_off + vl - kHalo / 2;
            if (use_window && wave >= 3)
                {
                    // two batches of loads in flight (the update hides their latency)
                    constexpr int kW = kTrkThreads - 192;
                    constexpr int kIt = (kWinCore + kHalo + kW - 1) / kW;
                    constexpr int kB = (kIt + 1) / 2;
                    // one 64-bit base per call and constant steps (per-item 64-bit
                    // offsets were hoisted out of the call loop and held 26 VGPRs)
                    const int i0 = tid - 192;
                    const int64_t g0 = nb + i0;
#pragma unroll
                    for (int j0 = 0; j0 < kIt; j0 += kB)
                        {
                            float2 wv[kB];
#pragma unroll
                            for (int j = 0; j < kB; ++j)
                                {
                                    const int64_t g = g0 + (int64_t)((j0 + j) * kW);
                                    wv[j] = (j0 + j < kIt && i0 + (j0 + j) * kW < kWinCore + kHalo && (uint64_t)g < iq_items)
                                                ? load_iq<IT>(iq, g)
                                                : make_float2(0.f, 0.f);
                                }
#pragma unroll
                            for (int j = 0; j < kB; ++j)
                                {
                                    const int i = i0 + (j0 + j) * kW;
                                    if (j0 + j < kIt && i < kWinCore + kHalo) s_win[i] = wv[j];
                                }
                        }
                }
            if (streamed)
                {
                    // chunks 0 and 1 of the call most likely next, into the two buffers,
                    // fetched by waves 3.. while wave 0 runs the loop update (its own
                    // memory waits stay unaffected) and waves 1 / 2 the speculative
                    // DLL/PLL and the EVM: the call's first in-call fetch is then chunk 2,
                    // issued a whole chunk of correlation ahead
                    const int64_t nb = p_off + vl - kHalo / 2;
                    const uint64_t nbytes = iq_items * (uint64_t)item_bytes<IT>();
                    // sized for the tail a last chunk may carry whatever this call's split
                    // (the buffers hold chunk + kTrkThreads + kHalo items): a call
                    // correlates the channel's constant vector_length samples
                    // (do_correlation_step, :1064-1076), so the split cannot change between
                    // calls today, but the prefetch no longer depends on that
                    const int pfn = (stream_chunk + kTrkThreads + kHalo) * item_bytes<IT>();
                    pf_start[0] = stream_fetch(iq, nbytes, nb * item_bytes<IT>(), pfn, s_sb, 3);
                    pf_start[1] = vl > stream_chunk + kTrkThreads
                                      ? stream_fetch(iq, nbytes, (nb + stream_chunk) * item_bytes<IT>(), pfn, s_sb + sbuf_bytes, 3)
                                      : 0;
                    pf_first = nb;
                }
            if (wave == 1)
                {
                    // this call's DLL/PLL on a copy of the state, into the code loop
                    // filter slot that is not current (take_dll_pll)
                    TrkHot t1 = s_t;
                    if (t1.state == 2 || t1.state == 4)
                        {
                            float2 taps[kMaxTrkTaps + 1], epl[3];
                            tap_totals(taps, epl);
                            const uint64_t n_read = t1.next_sample;
                            if (t1.pull_in_transitory &&
                                (n_read < c.acq_sample_stamp || n_read - c.acq_sample_stamp >= c.pull_in_span))
                                t1.pull_in_transitory = 0;
                            if (t1.state == 2)
                                {
                                    if (c.veml)
                                        {
                                            t1.VE_accu = taps[0];
                                            t1.VL_accu = taps[4];
                                        }
                                    t1.E_accu = epl[0];
                                    t1.P_accu = epl[1];
                                    t1.L_accu = epl[2];
                                    t1.spc = c.early_late_space_chips;
                                }
                            else
                                save_correlation_results(c, t1, taps, epl);
                            if constexpr (KF)
                                {
                                    // run_Kf (:1129-1166): discriminators, prediction and
                                    // P- H^T; then d_R -- in state 4 update_kf_cn0's, from
                                    // the C/N0 of this call's lock test (wave 2)
                                    KfShared* const ks = kf_shared<true>();
                                    const int cur = ks->cur;
                                    const KfModel km = kf_model(c.kf_beta, t1.corr_time);
                                    const double disc_hz = kf_carrier_disc(t1.cloop, t1.P_accu) / kTwoPi;
                                    const double disc_chips = c.veml ? dll_nc_vemlp(t1.VE_accu, t1.E_accu, t1.L_accu, t1.VL_accu)
                                                                     : kf_dll_nc_e_minus_l(t1.E_accu, t1.L_accu, t1.spc, 1.0F, 1.0F);
                                    const KfPred kp = kf_predict(km, ks->slot[cur], ks->q, lane);
                                    double R[2] = {ks->r[0], ks->r[1]};
                                    if (t1.state == 4)
                                        {
                                            while (__hip_atomic_load(&s_cn0_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) !=
                                                   (int)e)
                                                __builtin_amdgcn_s_sleep(1);
                                            kf_r_of_cn0(s_cn0.cn0_db_hz, t1.corr_time, t1.spc, R);
                                        }
                                    double K[2], xn[4];
                                    kf_gain(km, kp, R, disc_chips, disc_hz * kTwoPi, lane, K, xn);
                                    if (lane == 0)
                                        {
                                            KfSpec r;
                                            r.code_error_kf_chips = xn[0];
                                            r.carrier_phase_kf_rad = xn[1];
                                            r.carrier_doppler_kf_hz = xn[2];
                                            r.R[0] = R[0];
                                            r.R[1] = R[1];
                                            r.log_err[0] = (float)disc_hz;
                                            r.log_err[1] = (float)xn[2];
                                            r.log_err[2] = (float)disc_chips;
                                            r.log_err[3] = (float)xn[0];
                                            ks->spec = r;
                                            __hip_atomic_store(&s_spec_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                        }
                                    // off wave 0's path: the covariance, and the step into the
                                    // other slot (d_x_new_new(0) = 0, :1170)
                                    const double pn = kf_cov(km, kp, K, lane);
                                    KfSlot& nx = ks->slot[cur ^ 1];
                                    if (lane < 16) nx.P[lane] = pn;
                                    if (lane < 4) nx.x[lane] = lane == 0 ? 0.0 : (lane == 1 ? xn[1] : (lane == 2 ? xn[2] : xn[3]));
                                }
                            else
                                run_pll(c, t1);
                            if (!KF && lane == 0)
                                {
                                    DllPllSpec r;
                                    r.carrier_doppler_hz = t1.carrier_doppler_hz;
                                    r.P_accu_old = t1.P_accu_old;
                                    r.cf_w = t1.cf_w;
                                    r.cf_x = t1.cf_x;
                                    r.log_err[0] = t1.log_err[0];
                                    r.log_err[1] = t1.log_err[1];
                                    s_spec = r;
                                    __hip_atomic_store(&s_spec_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                            // then the EVM (an output only) with a full prompt buffer, which
                            // wave 0 takes for the record when the call stays locked: the
                            // buffer's other elements and this call's prompt (wave 2 writes
                            // only this call's element)
                            if (!KF && t1.cn0_estimation_counter >= c.cn0_samples)  // kf_tracking has no EVM
                                {
                                    const double evm = evm_of(c, t1.cn0_estimation_counter, t1.P_accu, s_pbuf, s_evm_buf, lane);
                                    if (lane == 0)
                                        {
                                            if (timing) s_w2t[2] = wall_clock64();
                                            s_evm = evm;
                                            __hip_atomic_store(&s_evm_e, (int)e, __ATOMIC_RELEASE,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
                                        }
                                }
                            // then the next call's plan from wave 0's state after its
                            // locked branch (wave 0 overrides it on a loss of lock)
                            while (__hip_atomic_load(&s_plan_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)e)
                                __builtin_amdgcn_s_sleep(1);
                            const PlanIn q = s_plan;
                            t1.carrier_phase_step_rad = q.carrier_phase_step_rad;
                            t1.carrier_phase_rate_step_rad = q.carrier_phase_rate_step_rad;
                            t1.rem_code_phase_chips = q.rem_code_phase_chips;
                            t1.code_phase_step_chips = q.code_phase_step_chips;
                            t1.code_phase_rate_step_chips = q.code_phase_rate_step_chips;
                            t1.next_sample = q.next_sample;
                            t1.rem_carr_phase_rad = q.rem_carr_phase_rad;
                            t1.state = q.state;
                            t1.narrow = q.narrow;
                            const Prep pn = make_prep(c, t1, e + 1 < max_epochs, iq_first, iq_items, vl, K, L, use_window,
                                streamed, stream_chunk, use_window ? nb : win_base, streamed ? nb : pf_first);
                            if (lane == 0)
                                {
                                    prep = pn;
                                    __hip_atomic_store(&s_prep_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                        }
                }
            if (wave == 2)
                {
                    // this call's lock test (CN0 estimate, lock detector, the prompt
                    // buffer) on a copy of the state, which wave 0 takes after its locked
                    // branch
                    TrkHot t2 = s_t;
                    if (t2.state == 2 || t2.state == 4)
                        {
                            float2 taps[kMaxTrkTaps + 1], epl[3];
                            tap_totals(taps, epl);
                            const uint64_t n_read = t2.next_sample;
                            if (t2.pull_in_transitory &&
                                (n_read < c.acq_sample_stamp || n_read - c.acq_sample_stamp >= c.pull_in_span))
                                {
                                    t2.pull_in_transitory = 0;
                                    t2.carrier_lock_fail_counter = 0;
                                    t2.code_lock_fail_counter = 0;
                                }
                            const double coh =
                                t2.state == 2 ? c.code_period : c.code_period * (double)c.extend_correlation_symbols;
                            pre_lock(c, t2, taps, epl, n_read);
                            if (timing && lane == 0) s_w2t[0] = wall_clock64();
                            const int locked = cn0_and_lock<KF>(c, t2, s_pbuf, s_cn, coh, lane);
                            if (lane == 0)
                                {
                                    if (timing) s_w2t[1] = wall_clock64();
                                    cn0_publish(s_cn0, t2, locked);
                                    __hip_atomic_store(&s_cn0_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                        }
                }
            if (wave == 0)
                {
                    TrkHot t = s_t;
                    uint64_t tmA = 0;
                    if (timing) tmA = wall_clock64();
                    float2 taps[kMaxTrkTaps + 1], epl[3];
                    tap_totals(taps, epl);
                    const uint64_t n_read = t.next_sample;
                    const int32_t state0 = t.state;
                    // pull-in transitory check at the top of general_work (:1794-1803):
                    // pull_in_time_s < (nitems_read - stamp) / (int)fs_in, integer division
                    if (t.pull_in_transitory &&
                        (n_read < c.acq_sample_stamp || n_read - c.acq_sample_stamp >= c.pull_in_span))
                        {
                            t.pull_in_transitory = 0;
                            t.carrier_lock_fail_counter = 0;
                            t.code_lock_fail_counter = 0;
                        }
                    EpochOut o;
                    uint64_t pr[3] = {0, 0, 0};
                    uint64_t tm3 = 0;
                    if (timing) tm3 = wall_clock64();
                    SpecLink sl{&s_spec, &s_dspec, &s_dspec_e, &s_spec_e, s_lfs, &s_lfi, lfi0, (int)e};
                    KfWave0<KF> kw;
                    (void)kw;
                    if constexpr (KF)
                        {
                            KfShared* const ks = kf_shared<true>();
                            kw.kfi0 = ks->cur;
                            kw.kl = KfLink{&ks->spec, &s_spec_e, ks->q, &s_cn0, &s_cn0_e, kw.kfi0, (int)e, {0.0, 0.0}};
                            after_correlation<true>(c, t, gc, kw.kl, taps, epl, n_read, o, timing != nullptr, pr);
                        }
                    else
                        after_correlation(c, t, gc, sl, taps, epl, n_read, o, timing != nullptr, pr);
                    t.next_sample = n_read + (uint64_t)(int64_t)t.current_prn_length_samples;
                    // the next call's plan (the window / chunk-0 prefetch of this iteration
                    // starts at nb): states 2 / 4 on wave 1 from the state published here,
                    // before the lock test's results (they change the plan only on a loss
                    // of lock: state 0, no call); state 3 here
                    const bool plan_w1 = state0 == 2 || state0 == 4;
                    Prep pn{};
                    if (plan_w1)
                        {
                            if (lane == 0)
                                {
                                    PlanIn q;
                                    q.carrier_phase_step_rad = t.carrier_phase_step_rad;
                                    q.carrier_phase_rate_step_rad = t.carrier_phase_rate_step_rad;
                                    q.rem_code_phase_chips = t.rem_code_phase_chips;
                                    q.code_phase_step_chips = t.code_phase_step_chips;
                                    q.code_phase_rate_step_chips = t.code_phase_rate_step_chips;
                                    q.next_sample = t.next_sample;
                                    q.rem_carr_phase_rad = t.rem_carr_phase_rad;
                                    q.state = t.state;
                                    q.narrow = t.narrow;
                                    s_plan = q;
                                    __hip_atomic_store(&s_plan_e, (int)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                        }
                    else
                        pn = make_prep(c, t, e + 1 < max_epochs, iq_first, iq_items, vl, K, L, use_window, streamed,
                            stream_chunk, use_window ? nb : win_base, streamed ? nb : pf_first);
                    bool lost = false;
                    uint64_t tjoin = 0;
                    if (state0 == 2 || state0 == 4)
                        {
                            if (timing) tjoin = wall_clock64();
                            while (__hip_atomic_load(&s_cn0_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)e)
                                __builtin_amdgcn_s_sleep(1);
                            const Cn0Spec r = s_cn0;
                            if (r.locked)
                                {
                                    cn0_apply(t, r);
                                    o.evm = !KF && r.locked == 2;
                                }
                            else
                                {
                                    // loss of lock: cn0_and_tracking_lock_status returned
                                    // false and the reference's call ends there (:1828-1845,
                                    // :2032-2040), so the locked branch above is void: the
                                    // call is rebuilt from its start state
                                    t = s_t;
                                    if (t.pull_in_transitory &&
                                        (n_read < c.acq_sample_stamp || n_read - c.acq_sample_stamp >= c.pull_in_span))
                                        t.pull_in_transitory = 0;
                                    pre_lock(c, t, taps, epl, n_read);
                                    cn0_apply(t, r);
                                    if constexpr (KF)
                                        {
                                            // kf_tracking::clear_tracking_vars (:1217-1233) leaves
                                            // the discriminator and filter outputs that log_data
                                            // dumps as they are; the filter step is dropped
                                            float le[4];
                                            for (int i = 0; i < 4; ++i) le[i] = t.log_err[i];
                                            clear_tracking_vars(t);
                                            for (int i = 0; i < 4; ++i) t.log_err[i] = le[i];
                                            kw.kl.kfi = kw.kfi0;
                                        }
                                    else
                                        clear_tracking_vars(t);
                                    if (c.track_pilot) t.P_data_accu = make_float2(0.f, 0.f);
                                    t.state = 0;
                                    init_out(o);
                                    o.flags = GSDR_TRK_F_LOSS_OF_LOCK | (t.flag_pll_180 ? GSDR_TRK_F_PLL_180 : 0);
                                    sl.lfi = lfi0;  // the DLL/PLL results were not taken
                                    t.next_sample = n_read + (uint64_t)(int64_t)t.current_prn_length_samples;
                                    lost = true;
                                }
                        }
                    if (sl.lfi != lfi0)
                        {
                            lfi0 = sl.lfi;
                            if (lane == 0) s_lfi = lfi0;
                        }
                    if constexpr (KF)
                        {
                            if (kw.kl.kfi != kw.kfi0)
                                {
                                    if (lane == 0)
                                        {
                                            KfShared* const ks = kf_shared<true>();
                                            ks->cur = kw.kl.kfi;
                                            ks->r[0] = kw.kl.R[0];
                                            ks->r[1] = kw.kl.R[1];
                                        }
                                }
                        }
                    uint64_t tevm0 = 0, tevm1 = 0;
                    if (o.evm)
                        {
                            if (timing) tevm0 = wall_clock64();
                            while (__hip_atomic_load(&s_evm_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)e)
                                __builtin_amdgcn_s_sleep(1);
                            t.evm = s_evm;
                            if (timing) tevm1 = wall_clock64();
                        }
                    if (lane == 0)
                        {
                            gsdr_trk_epoch r;
                            r.sample_counter = n_read;
                            r.state = state0;
                            r.consumed = t.current_prn_length_samples;
#pragma unroll
                            for (int k = 0; k < 5; ++k)
                                {
                                    r.taps[2 * k] = taps[k].x;
                                    r.taps[2 * k + 1] = taps[k].y;
                                }
                            r.rem_carr_phase_rad = t.rem_carr_phase_rad;
                            r.flags = o.flags;
                            r.carrier_doppler_hz = t.carrier_doppler_hz;
                            r.code_freq_chips = t.code_freq_chips;
                            r.rem_code_phase_samples = t.rem_code_phase_samples;
                            r.acc_carrier_phase_rad = t.acc_carrier_phase_rad;
                            r.cn0_db_hz = t.cn0_db_hz;
                            r.carrier_lock_test = t.carrier_lock_test;
                            r.prompt_i = o.prompt_i;
                            r.prompt_q = o.prompt_q;
                            r.evm = t.evm;
                            r.data_prompt[0] = data ? taps[kMaxTrkTaps].x : 0.0F;
                            r.data_prompt[1] = data ? taps[kMaxTrkTaps].y : 0.0F;
                            r.carrier_rate = (float)t.carrier_phase_rate_step_rad;
                            r.code_rate = (float)t.code_phase_rate_step_chips;
#pragma unroll
                            for (int i = 0; i < 5; ++i) r.log_accu[i] = o.log_accu[i];
                            r.carr_phase_error_hz = t.log_err[0];
                            r.carr_error_filt_hz = t.log_err[1];
                            r.code_error_chips = t.log_err[2];
                            r.code_error_filt_chips = t.log_err[3];
                            r.reserved = 0;
                            out[(size_t)ch * max_epochs + e] = r;
                            if (timing)
                                {
                                    uint64_t* tr = timing + ((size_t)ch * max_epochs + e) * kTimingSlots;
                                    tr[0] = tm0;
                                    tr[1] = tm1;
                                    tr[2] = tm2;
                                    tr[3] = tmA;
                                    tr[4] = tm3;
                                    tr[5] = pr[0] ? pr[0] : tm3;
                                    tr[6] = pr[1] ? pr[1] : tr[5];
                                    tr[7] = pr[2] ? pr[2] : tr[6];
                                    tr[8] = wall_clock64();
                                    tr[10] = swait;
                                    const bool w2 = tjoin != 0;
                                    tr[11] = w2 && s_w2t[0] >= tm2 ? s_w2t[0] - tm2 : 0;
                                    tr[12] = w2 && s_w2t[1] >= tm2 ? s_w2t[1] - tm2 : 0;
                                    tr[13] = w2 && tjoin >= tm2 ? tjoin - tm2 : 0;
                                    tr[14] = tevm0 && s_w2t[2] >= tm2 ? s_w2t[2] - tm2 : 0;
                                    tr[15] = tevm0 >= tm2 && tevm0 ? tevm0 - tm2 : 0;
                                    tr[16] = tevm1 >= tm2 && tevm1 ? tevm1 - tm2 : 0;
                                }
                        }
                    if (lane == 0) s_t = t;
                    if (!plan_w1)
                        {
                            if (lane == 0) prep = pn;
                        }
                    else if (lost)
                        {
                            // no next call: after wave 1's plan, so this write lands last
                            while (__hip_atomic_load(&s_prep_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)e)
                                __builtin_amdgcn_s_sleep(1);
                            if (lane == 0) prep.go = 0;
                        }
                    if (timing && lane == 0) timing[((size_t)ch * max_epochs + e) * kTimingSlots + 9] = wall_clock64();
                }
            if (use_window) win_base = nb;
            // the next iteration's prep barrier orders the window writes and s_red reuse
        }
    __syncthreads();
    if (tid == 0)
        {
            gc->h = s_t;
            gc->code_filter = s_lfs[s_lfi];
            nout[ch] = e + (uint32_t)s_overrun;
        }
    if (tid < kMaxCn0) gc->prompt_buffer[tid] = s_pbuf[tid];
    if constexpr (KF)
        {
            KfShared* const ks = kf_shared<true>();
            const KfSlot& cur = ks->slot[ks->cur];
            if (tid < 16) gc->kf.P[tid] = cur.P[tid];
            if (tid < 16) gc->kf.Q[tid] = ks->q[tid];
            if (tid < 4) gc->kf.x[tid] = cur.x[tid];
            if (tid < 2) gc->kf.R[tid] = ks->r[tid];
        }
}

}  // namespace
