// Tracking: what the host unit (trk.hip) and the kernel units (trk_dll_pll.hip, trk_kf.hip)
// share -- the capacity and tiling constants, the layouts that cross the host/device line,
// the kernel pointer type and the kernel units' getters.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsdr_internal.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

namespace gsdr
{
namespace trk
{

#ifndef GSDR_TRK_THREADS
#define GSDR_TRK_THREADS 512
#endif
constexpr int kTrkThreads = GSDR_TRK_THREADS;
constexpr int kMaxCn0 = 64;         // cn0_samples capacity
constexpr int kMaxTrkTaps = 5;
constexpr int kMaxCodeFloats = 16384;
constexpr int kPreambleLen = 160;   // GPS_CA_PREAMBLE_LENGTH_SYMBOLS (GPS_L1_CA.h:61)
constexpr int kMaxSmoother = 32;             // Dll_Pll_Conf::smoother_length cap (high_dyn histories)
#ifndef GSDR_TRK_SPL
#define GSDR_TRK_SPL 8
#endif
constexpr int kSpl = GSDR_TRK_SPL;            // samples per lane per correlation chunk
constexpr int kWinCore = kSpl * kTrkThreads;  // 4096: the next call's window staged in LDS
constexpr int kHalo = 16;                     // slack around the predicted next start
constexpr int kStreamRow = 64 * 16;           // bytes one wave's global_load_lds_dwordx4 writes
constexpr int kCodeMargin = 32;              // replica samples copied on each side of the LDS replica
constexpr int kTimingSlots = 17;             // GSDR_TRK_TIMING record per call: 10 stamps + stream-wait ticks
                                             // + wave 2's lock test start / end and wave 0's
                                             // arrival at the join, wave 1's EVM end, wave 0 at the EVM
                                             // join and after it, as offsets from the partials barrier
constexpr int kStampSlots = 10;

// MATH_CONSTANTS.h:47-50
constexpr double kGnssPi = 3.1415926535898;
constexpr double kTwoPi = 2.0 * kGnssPi;
constexpr double kHalfPi = kGnssPi / 2.0;

struct LoopFilter  // Tracking_loop_filter (tracking_loop_filter.cc)
{
    float inputs[4], outputs[4], icoef[4], ocoef[3];
    int nin, nout, idx, order;
    float bw, T;
};

// Per-channel configuration: read-only inside the kernel (a separate restrict
// array, so its fields are fetched with scalar loads into SGPRs).
struct CfConst  // Tracking_FLL_PLL_filter coefficients
{
    float w0p3, w0f2, a2, w0f, a3, w0p2, b3, w0p;
    int order;
};

struct SmConst  // Exponential_Smoother parameters
{
    float alpha, one_minus_alpha, min_value, offset;
    int samples_init;
};

struct TrkConst
{
    double fs_in, code_period, code_chip_rate, signal_carrier_freq, carrier_lock_threshold;
    uint64_t acq_sample_stamp;
    uint64_t pull_in_span;   // (pull_in_time_s + 1) * (int)fs_in: the integer-second test of :1797 flips there
    uint64_t bit_sync_span;  // (bit_synchronization_time_limit_s + 1) * (int)fs_in (:1866)
    float early_late_space_chips;
    float shifts[kMaxTrkTaps];
    uint32_t preamble[5];    // secondary code / preamble as the circular-buffer register (acquire_secondary)
    uint32_t sec_str[5];     // secondary code string bit i = (code[i] == '1') (state-4 wipe-off)
    uint32_t data_sec_str;   // data secondary code (BeiDou NH), same form
    int32_t sec_len, data_sec_len, secondary, veml, track_pilot, iE, iP, iL;
    // extended coherent integration (state 3, :1945-1983): narrow taps, loops, time
    float shifts_narrow[kMaxTrkTaps];
    float early_late_space_narrow_chips, dll_bw_narrow_hz;
    double corr_time_ext;
    int32_t enable_ext;
    int32_t vector_length, code_length_chips, code_samples_per_chip, symbols_per_bit;
    int32_t cn0_samples, cn0_min, max_code_lock_fail, max_carrier_lock_fail;
    int32_t extend_correlation_symbols, enable_fll_pull_in, enable_fll_steady_state, carrier_aiding;
    int32_t n_taps, code_samples;
    uint32_t prn;
    CfConst cf;
    SmConst sm[2];  // 0: CN0, 1: carrier lock test
    CfConst cf_narrow;
    int32_t high_dyn, smoother_length;  // Dll_Pll_Conf::high_dyn / smoother_length (dll_pll_conf.h:62,80)
    int32_t interchange_iq;  // d_interchange_iq (:242, :310): Prompt_I / Prompt_Q swapped on output
    double kf_beta;          // Kalman loop: d_beta = d_code_chip_rate / d_signal_carrier_freq (kf_tracking.cc:448)
};

// Mutable scalar loop state (dll_pll_veml_tracking.h:117-209 minus the
// per-call temporaries): in wave 0's registers for a whole launch.
struct TrkHot
{
    double code_freq_chips, carrier_doppler_hz, acc_carrier_phase_rad, rem_code_phase_chips;
    double carrier_lock_test, cn0_db_hz, evm;
    double carrier_phase_step_rad, carrier_phase_rate_step_rad, code_phase_step_chips, code_phase_rate_step_chips;
    double rem_code_phase_samples;
    uint64_t next_sample;
    float2 VE_accu, E_accu, P_accu, P_accu_old, L_accu, VL_accu, P_data_accu;
    float cf_w, cf_x;                  // Tracking_FLL_PLL_filter state
    float sm_old[2], sm_sum[2];        // smoothers: value and running init sum
    int32_t sm_counter[2], sm_init[2];
    uint32_t circ[5];                  // signs of the last kPreambleLen prompts (1 = real < 0), newest at bit 0
    int32_t circ_size;
    float rem_carr_phase_rad, spc;
    int32_t state, current_prn_length_samples, current_symbol, current_data_symbol, cn0_estimation_counter;
    int32_t carrier_lock_fail_counter, code_lock_fail_counter;
    int32_t pull_in_transitory, cloop, acc_carrier_phase_initialized, flag_pll_180;
    double corr_time;            // d_current_correlation_time_s
    int32_t narrow, extend_count;  // after the switch to the extended correlator
    int32_t hist_n, hist_head;     // high_dyn: d_carr_ph_history / d_code_ph_history fill and oldest slot
    // run_dll_pll's d_carr_phase_error_hz, d_carr_error_filt_hz, d_code_error_chips,
    // d_code_error_filt_chips as log_data writes them (float of the double members)
    float log_err[4];
};

// Kalman loop (kf_tracking.h:121-130): the filter's state of one channel.  d_F and d_H are
// functions of d_current_correlation_time_s (TrkHot::corr_time) alone and are rebuilt from
// it every call (kf_model); d_R is diagonal.
struct TrkKf
{
    double x[4];   // d_x_old_old: code-phase error [chips], carrier phase [rad], Doppler [Hz], rate [Hz/s]
    double P[16];  // d_P_old_old, row-major
    double Q[16];  // d_Q (update_kf_narrow_integration_time replaces it)
    double R[2];   // d_R(0,0), d_R(1,1)
};

// Device-memory image of the mutable part of one channel.
struct TrkChan
{
    TrkHot h;
    LoopFilter code_filter;
    float2 prompt_buffer[kMaxCn0];
    // high_dyn: the two boost::circular_buffer<pair<double,double>> of capacity
    // 2*smoother_length (:554-563), pushed together (same sample count)
    double hist_carr[2 * kMaxSmoother], hist_code[2 * kMaxSmoother], hist_samples[2 * kMaxSmoother];
    TrkKf kf;  // Kalman mode only (gsdr_trk_set_kf)
};

// the kernel instance of an item type and replica layout
using TrkKernel = void (*)(const TrkConst*, TrkChan*, const float* const*, const float* const*, const void*, uint64_t, uint64_t,
    uint32_t, gsdr_trk_epoch*, uint32_t*, int, int, uint64_t*, int, int, int);

}  // namespace trk

// the six DLL/PLL-loop instances (trk_dll_pll.hip) and the six Kalman-loop ones (trk_kf.hip)
trk::TrkKernel trk_dll_pll_kernel(int item_type, bool pack);
trk::TrkKernel trk_kf_kernel(int item_type, bool pack);
}  // namespace gsdr

namespace
{
using namespace gsdr::trk;

__host__ __device__ inline void lf_update(LoopFilter& f)  // :98-197
{
    float g1, g2, g3, wn;
    const float T = f.T;
    const float zeta = 1.0F / sqrtf(2.0F);
    switch (f.order)
        {
        case 1:
            wn = f.bw * 4.0F;
            g1 = wn;
            f.nin = 1;
            f.icoef[0] = g1;
            f.nout = 0;
            break;
        case 2:
            wn = f.bw * (8.0F * zeta) / (4.0F * zeta * zeta + 1.0F);
            g1 = wn * wn;
            g2 = wn * 2.0F * zeta;
            f.nin = 2;
            f.icoef[0] = (float)(g1 * T / 2.0 + g2);
            f.icoef[1] = (float)(g1 * T / 2.0 - g2);
            f.nout = 1;
            f.ocoef[0] = 1.0F;
            break;
        default:
            {
                wn = f.bw / 0.7845F;
                const float a3 = 1.1F, b3 = 2.4F;
                g1 = wn * wn * wn;
                g2 = a3 * wn * wn;
                g3 = b3 * wn;
                f.nin = 3;
                f.icoef[0] = (float)(g3 + T / 2.0 * (g2 + T / 2.0 * g1));
                f.icoef[1] = (float)(g1 * T * T / 2.0 - 2.0 * g3);
                f.icoef[2] = (float)(g3 + T / 2.0 * (-g2 + T / 2.0 * g1));
                f.nout = 2;
                f.ocoef[0] = 2.0F;
                f.ocoef[1] = -1.0F;
            }
            break;
        }
}

__host__ __device__ inline void lf_initialize(LoopFilter& f, float y0)  // :258-263
{
    for (int i = 0; i < 4; ++i)
        {
            f.inputs[i] = 0.0F;
            f.outputs[i] = y0;
        }
    f.idx = 3;
}

__host__ __device__ inline void sm_reset(TrkHot& t, int w)
{
    t.sm_init[w] = 1;
    t.sm_counter[w] = 0;
    t.sm_sum[w] = 0.0F;
}

}  // namespace
