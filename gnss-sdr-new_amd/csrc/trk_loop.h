// Tracking: the loop library and wave 0's loop update of the DLL/PLL loop -- loop filter,
// discriminators, cn0_and_lock, run_pll / run_dll, update_tracking_vars, acquire_secondary,
// save_correlation_results, the hand-offs between the waves and after_correlation.
// after_correlation<true> names take_kf and kf_narrow of trk_kf_step.h; they are looked up
// where the template is instantiated (trk_kernel.h), so this header needs no Kalman one.
#pragma once
#include "trk_types.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

namespace
{
using namespace gsdr::trk;

// ------------------------------------------------------------------ loop library
// Tracking_loop_filter::apply on a filter held in registers (wave 3's speculative
// DLL/PLL): the ring elements are separate scalars picked by selects -- with arrays
// the compiler turned the selects back into a run-time index, i.e. a scratch access
// (and the LDS form was a chain of dependent LDS round trips).  The reference's
// products and sums in its order.
struct LfReg
{
    float i0, i1, i2, i3, o0, o1, o2, o3, c0, c1, c2, c3, d0, d1, d2;
    int nin, nout, idx;
};

__device__ __forceinline__ LfReg lf_load(const LoopFilter& f)
{
    return LfReg{f.inputs[0], f.inputs[1], f.inputs[2], f.inputs[3], f.outputs[0], f.outputs[1], f.outputs[2],
        f.outputs[3], f.icoef[0], f.icoef[1], f.icoef[2], f.icoef[3], f.ocoef[0], f.ocoef[1], f.ocoef[2], f.nin, f.nout,
        f.idx};
}

__device__ __forceinline__ float lf_pick(float a0, float a1, float a2, float a3, int i)
{
    return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3));
}

__device__ __forceinline__ float lf_apply(LfReg& f, float in)  // :58-93
{
    float r = 0.0F;
    const float oc[3] = {f.d0, f.d1, f.d2};
    const float ic[4] = {f.c0, f.c1, f.c2, f.c3};
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
        if (ii < f.nout) r += oc[ii] * lf_pick(f.o0, f.o1, f.o2, f.o3, (f.idx + ii) & 3);
    f.idx--;
    if (f.idx < 0) f.idx += 4;
    f.i0 = f.idx == 0 ? in : f.i0;
    f.i1 = f.idx == 1 ? in : f.i1;
    f.i2 = f.idx == 2 ? in : f.i2;
    f.i3 = f.idx == 3 ? in : f.i3;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
        if (ii < f.nin) r += ic[ii] * lf_pick(f.i0, f.i1, f.i2, f.i3, (f.idx + ii) & 3);
    f.o0 = f.idx == 0 ? r : f.o0;
    f.o1 = f.idx == 1 ? r : f.o1;
    f.o2 = f.idx == 2 ? r : f.o2;
    f.o3 = f.idx == 3 ? r : f.o3;
    return r;
}

// ------------------------------------------------------------------ wave-0 loop body
// The loop update runs on all 64 lanes of wave 0 with identical (uniform)
// values; the loops over the CN0 buffer put one element on each lane and sum in
// the reference's element order with readlane, so results are bit-identical to
// the sequential code.  Memory writes are done by lane 0.
__device__ __forceinline__ float lane_f(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }

__device__ inline float cf_error(const CfConst& k, TrkHot& t, float fll, float pll, float tc)  // :77-101
{
    float e;
    if (k.order == 3)
        {
            t.cf_w = t.cf_w + tc * (k.w0p3 * pll + k.w0f2 * fll);
            t.cf_x = t.cf_x + tc * (0.5F * t.cf_w + k.a2 * k.w0f * fll + k.a3 * k.w0p2 * pll);
            e = 0.5F * t.cf_x + k.b3 * k.w0p * pll;
        }
    else
        {
            const float wn = t.cf_w + pll * k.w0p2 * tc + fll * k.w0f * tc;
            e = 0.5F * (wn + t.cf_w) + k.a2 * k.w0p * pll;
            t.cf_w = wn;
        }
    return e;
}

__device__ inline float sm_smooth(const SmConst& k, TrkHot& t, int w, float raw)  // exponential_smoother.cc:84-110
{
    float v;
    if (t.sm_init[w])
        {
            t.sm_counter[w]++;
            v = raw;
            t.sm_sum[w] = t.sm_sum[w] + v;
            if (t.sm_counter[w] == k.samples_init)
                {
                    t.sm_old[w] = t.sm_sum[w] / (float)t.sm_counter[w];
                    if (t.sm_old[w] < (k.min_value + k.offset))
                        {
                            t.sm_counter[w] = 0;
                            t.sm_sum[w] = 0.0F;
                        }
                    else
                        t.sm_init[w] = 0;
                }
        }
    else
        {
            v = k.alpha * raw + k.one_minus_alpha * t.sm_old[w];
            t.sm_old[w] = v;
        }
    return v;
}

__device__ inline double pll_cloop_two_quadrant_atan(float2 p)  // tracking_discriminators.cc:92-99
{
    if (p.x != 0.0F) return (double)atanf(p.y / p.x);
    return 0.0;
}

__device__ inline double phase_unwrap(double p)
{
    if (p >= kHalfPi) return p - kGnssPi;
    if (p <= -kHalfPi) return p + kGnssPi;
    return p;
}

__device__ inline double fll_diff_atan(float2 s1, float2 s2, double t1, double t2)  // :62-70
{
    double d = (double)(atanf(s2.y / s2.x) - atanf(s1.y / s1.x));
    if (isnan(d)) d = 0;
    return phase_unwrap(d) / (t2 - t1);
}

__device__ inline double dll_nc_e_minus_l(float2 e, float2 l, float spc, float slope, float y)  // :110-120
{
    const double pe = (double)hypotf(e.x, e.y);
    const double pl = (double)hypotf(l.x, l.y);
    const double s = pe + pl;
    if (s == 0.0) return 0.0;
    return (double)((y - slope * spc) / slope) * (pe - pl) / s;
}

// pll_four_quadrant_atan (:86-89); gr::fast_atan2f restated as atan2f
__device__ inline double pll_four_quadrant_atan(float2 p) { return (double)atan2f(p.y, p.x); }

__device__ inline double dll_nc_vemlp(float2 ve, float2 e, float2 l, float2 vl)  // :139-149
{
    const double Early = sqrt((double)(ve.x * ve.x + ve.y * ve.y + e.x * e.x + e.y * e.y));
    const double Late = sqrt((double)(l.x * l.x + l.y * l.y + vl.x * vl.x + vl.y * vl.y));
    const double s = Early + Late;
    if (s == 0.0) return 0.0;
    return (Early - Late) / s;
}

__device__ inline void clear_tracking_vars(TrkHot& t)  // :1192-1213
{
    t.P_accu_old = make_float2(0.f, 0.f);
    t.current_symbol = 0;
    t.current_data_symbol = 0;
    t.circ_size = 0;
    for (int w = 0; w < 5; ++w) t.circ[w] = 0u;
    t.carrier_phase_rate_step_rad = 0.0;
    t.code_phase_rate_step_chips = 0.0;
    t.hist_n = 0;  // d_carr_ph_history.clear(), d_code_ph_history.clear()
    t.hist_head = 0;
    for (int i = 0; i < 4; ++i) t.log_err[i] = 0.0F;
}

// Sequential float sums over the buffer elements (the estimators' loops, in the
// reference's element order): every lane of wave 0 reads the per-element terms
// back from LDS (same address on all lanes) and adds them in order.
template <int NS>
__device__ __forceinline__ void seq_sums(const float* terms, int stride, int n, float (&sum)[NS])
{
    __builtin_amdgcn_wave_barrier();
    for (int q = 0; q < NS; ++q) sum[q] = 0.0F;
    int i = 0;
    for (; i + 4 <= n; i += 4)
        {
            float4 v[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) v[q] = *reinterpret_cast<const float4*>(terms + q * stride + i);
#pragma unroll
            for (int q = 0; q < NS; ++q) sum[q] += v[q].x;
#pragma unroll
            for (int q = 0; q < NS; ++q) sum[q] += v[q].y;
#pragma unroll
            for (int q = 0; q < NS; ++q) sum[q] += v[q].z;
#pragma unroll
            for (int q = 0; q < NS; ++q) sum[q] += v[q].w;
        }
    for (; i < n; ++i)
#pragma unroll
        for (int q = 0; q < NS; ++q) sum[q] += terms[q * stride + i];
}

// cn0_and_tracking_lock_status (:970-1056) with cn0_m2m4_estimator and
// carrier_lock_detector (lock_detectors.cc:90-148); wave 2 on its copy of the
// call's state (Cn0Spec), lane = element,
// sums in element order through `scratch` (3 x kMaxCn0 floats of LDS).  Returns 0 on a
// loss of lock, 1 while the prompt buffer fills, 2 with a full buffer: then the EVM
// (:1027-1053, an output only) is the one wave 1 computes (evm_of).
// CR: the Kalman loop's form.  Its filter integrates what the float library functions of a
// call return without decay (x(1) never wraps, and in a replay nothing feeds back), so a last
// place of log10f, atanf or hypotf, which no two libraries agree on, stays in x and P for
// good.  There these functions are evaluated correctly rounded -- in double, rounded to
// float -- which is one definite value on every platform (kf_restatement.py does the same).
template <bool CR = false>
__device__ inline int cn0_and_lock(const TrkConst& c, TrkHot& t, float2* pbuf, float (*scratch)[kMaxCn0], double coh,
    int lane)
{
    const int n = c.cn0_samples;
    if (t.cn0_estimation_counter < n)
        {
            if (lane == 0) pbuf[t.cn0_estimation_counter] = t.P_accu;
            t.cn0_estimation_counter++;
            return 1;
        }
    const int widx = t.cn0_estimation_counter % n;
    float2 ei = make_float2(0.f, 0.f);
    if (lane < n) ei = lane == widx ? t.P_accu : pbuf[lane];
    if (lane == 0) pbuf[widx] = t.P_accu;
    t.cn0_estimation_counter++;
    // cn0_m2m4_estimator: Psig += |re|; aux = im*im + re*re; m2 += aux; m4 += aux*aux
    const float a_i = fabsf(ei.x);
    const float aux_i = ei.y * ei.y + ei.x * ei.x;
    const float aux2_i = aux_i * aux_i;
    scratch[0][lane] = a_i;
    scratch[1][lane] = aux_i;
    scratch[2][lane] = aux2_i;
    float sums[3];
    seq_sums<3>(&scratch[0][0], kMaxCn0, n, sums);
    float psig = sums[0], m2 = sums[1], m4 = sums[2];
    const float fn = (float)n;
    psig /= fn;
    psig = psig * psig;
    m2 /= fn;
    m4 /= fn;
    float aux = sqrtf(2.0F * m2 * m2 - m4);
    float snr;
    if (isnan(aux))
        snr = psig / (m2 - psig);
    else
        snr = aux / (m2 - aux);
    float raw;
    if constexpr (CR)
        raw = 10.0F * (float)log10((double)snr) - 10.0F * (float)log10((double)(float)coh);
    else
        raw = 10.0F * log10f(snr) - 10.0F * log10f((float)coh);
    t.cn0_db_hz = (double)sm_smooth(c.sm[0], t, 0, raw);
    // carrier_lock_detector(buffer, 1): element 0 only
    const float si = 0.0F + lane_f(ei.x, 0), sq = 0.0F + lane_f(ei.y, 0);
    const float lock = (si * si - sq * sq) / (si * si + sq * sq);
    t.carrier_lock_test = (double)sm_smooth(c.sm[1], t, 1, lock);
    if (!t.pull_in_transitory)
        {
            if (t.carrier_lock_test < c.carrier_lock_threshold)
                t.carrier_lock_fail_counter++;
            else if (t.carrier_lock_fail_counter > 0)
                t.carrier_lock_fail_counter--;
            if (t.cn0_db_hz < c.cn0_min)
                t.code_lock_fail_counter++;
            else if (t.code_lock_fail_counter > 0)
                t.code_lock_fail_counter--;
        }
    if (t.carrier_lock_fail_counter > c.max_carrier_lock_fail || t.code_lock_fail_counter > c.max_code_lock_fail)
        {
            t.carrier_lock_fail_counter = 0;
            t.code_lock_fail_counter = 0;
            return 0;
        }
    return 2;
}

// The fork indicator EVM of cn0_and_tracking_lock_status (:1027-1053) on wave 1, from
// the prompt buffer with this call's prompt (a full buffer: cn0_estimation_counter >=
// cn0_samples before the call): the same float sums in element order as the oracle,
// through `scratch` (2 x kMaxCn0 floats of LDS).
__device__ inline double evm_of(const TrkConst& c, int cn0_counter, float2 p_accu, const float2* pbuf, float* scratch,
    int lane)
{
    const int n = c.cn0_samples;
    const int widx = cn0_counter % n;
    float2 ei = make_float2(0.f, 0.f);
    if (lane < n) ei = lane == widx ? p_accu : pbuf[lane];
    scratch[lane] = ei.x * ei.x;  // sum of squared in-phase prompts
    float s1[1];
    seq_sums<1>(scratch, 0, n, s1);
    const float fn = (float)n;
    float d = s1[0] / fn;
    d = sqrtf(d);
    const float ea = fabsf(ei.x / d) - 1.0F;
    const float eb = fabsf(ei.y / d) - 0.0F;
    const float aa_i = ea * ea, bb_i = eb * eb;
    __builtin_amdgcn_wave_barrier();
    scratch[2 * lane] = aa_i;  // interleaved: s = s + aa_i; s = s + bb_i in element order
    scratch[2 * lane + 1] = bb_i;
    float s2[1];
    seq_sums<1>(scratch, 0, 2 * n, s2);
    return sqrt((double)(s2[0] / fn / 1.0F));
}

// run_dll_pll (:1092-1179, no Doppler correction) as its two independent halves, on
// two waves: the carrier loop (PLL / FLL discriminators and filter) and the code loop
// (DLL discriminator and filter); the carrier aiding term, the one product of the two,
// is added where they are joined (take_dll_pll), in the reference's order
__device__ inline void run_pll(const TrkConst& c, TrkHot& t)
{
    const double carr_phase_error_hz =
        (t.cloop ? pll_cloop_two_quadrant_atan(t.P_accu) : pll_four_quadrant_atan(t.P_accu)) / kTwoPi;
    double carr_error_filt_hz;
    if ((t.pull_in_transitory && c.enable_fll_pull_in) || c.enable_fll_steady_state)
        {
            const double carr_freq_error_hz = fll_diff_atan(t.P_accu_old, t.P_accu, 0, t.corr_time) / kTwoPi;
            t.P_accu_old = t.P_accu;
            if (t.pull_in_transitory && c.enable_fll_pull_in)
                carr_error_filt_hz = (double)cf_error(t.narrow ? c.cf_narrow : c.cf, t, (float)carr_freq_error_hz, 0.0F,
                    (float)t.corr_time);
            else
                carr_error_filt_hz = (double)cf_error(t.narrow ? c.cf_narrow : c.cf, t, (float)carr_freq_error_hz, (float)carr_phase_error_hz,
                    (float)t.corr_time);
        }
    else
        {
            carr_error_filt_hz = (double)cf_error(t.narrow ? c.cf_narrow : c.cf, t, 0, (float)carr_phase_error_hz, (float)t.corr_time);
        }
    t.carrier_doppler_hz = carr_error_filt_hz;
    t.log_err[0] = (float)carr_phase_error_hz;
    t.log_err[1] = (float)carr_error_filt_hz;
}

// the code loop's d_code_freq_chips before the carrier aiding term
__device__ inline double run_dll(const TrkConst& c, TrkHot& t, LfReg& lf)
{
    const double code_error_chips =
        c.veml ? dll_nc_vemlp(t.VE_accu, t.E_accu, t.L_accu, t.VL_accu) : dll_nc_e_minus_l(t.E_accu, t.L_accu, t.spc, 1.0F, 1.0F);
    const double code_error_filt_chips = (double)lf_apply(lf, (float)code_error_chips);
    t.log_err[2] = (float)code_error_chips;
    t.log_err[3] = (float)code_error_filt_chips;
    return c.code_chip_rate - code_error_filt_chips;
}

// high_dyn rate estimate (:1232-1251, :1265-1284): mean of the newest
// smoother_length steps minus mean of the oldest, over the newest sample counts,
// summed in the reference's order ([k] counts from the oldest element).  The
// element just pushed (slot) comes from registers, not read back.
__device__ inline double hist_rate(const double* v, const double* s, int head, int cap, int L, int slot, double vnew,
    double snew)
{
    double cp1 = 0.0, cp2 = 0.0, samples = 0.0;
    for (int k = 0; k < L; ++k)
        {
            const int a = (head + k) % cap, b = (head + 2 * L - k - 1) % cap;
            cp1 += a == slot ? vnew : v[a];
            cp2 += b == slot ? vnew : v[b];
            samples += b == slot ? snew : s[b];
        }
    cp1 /= (double)L;
    cp2 /= (double)L;
    return (cp2 - cp1) / samples;
}

// Every lane of wave 0 runs this with uniform values; the history stores write
// the same value from every lane.
// KF: kf_tracking::update_tracking_vars (kf_tracking.cc:1237-1313), the same but for the
// accumulated carrier phase, from which it subtracts the float remnant (:1279-1284)
template <bool KF = false>
__device__ inline void update_tracking_vars(const TrkConst& c, TrkHot& t, TrkChan* gc)  // :1216-1287
{
    const double T_chip = 1.0 / t.code_freq_chips;
    const double T_prn = T_chip * (double)c.code_length_chips;
    const double T_prn_samples = T_prn * c.fs_in;
    const double K_blk = T_prn_samples + t.rem_code_phase_samples;
    t.current_prn_length_samples = (int32_t)floor(K_blk);
    t.carrier_phase_step_rad = kTwoPi * t.carrier_doppler_hz / c.fs_in;
    int slot = 0;
    const int cap = 2 * c.smoother_length;
    const double ns = (double)t.current_prn_length_samples;
    if (c.high_dyn)
        {
            // push_back on a full circular buffer overwrites the oldest element
            if (t.hist_n < cap)
                {
                    slot = (t.hist_head + t.hist_n) % cap;
                    t.hist_n++;
                }
            else
                {
                    slot = t.hist_head;
                    t.hist_head = (t.hist_head + 1) % cap;
                }
            if (t.hist_n == cap)
                t.carrier_phase_rate_step_rad = hist_rate(gc->hist_carr, gc->hist_samples, t.hist_head, cap,
                    c.smoother_length, slot, t.carrier_phase_step_rad, ns);
            gc->hist_carr[slot] = t.carrier_phase_step_rad;
        }
    const double len = (double)t.current_prn_length_samples;
    t.rem_carr_phase_rad += (float)(t.carrier_phase_step_rad * len + 0.5 * t.carrier_phase_rate_step_rad * len * len);
    t.rem_carr_phase_rad = (float)fmod((double)t.rem_carr_phase_rad, kTwoPi);
    if constexpr (KF)
        t.acc_carrier_phase_rad -=
            (double)(float)(t.carrier_phase_step_rad * len + 0.5 * t.carrier_phase_rate_step_rad * len * len);
    else
        t.acc_carrier_phase_rad -= (t.carrier_phase_step_rad * len + 0.5 * t.carrier_phase_rate_step_rad * len * len);
    t.code_phase_step_chips = t.code_freq_chips / c.fs_in;
    if (c.high_dyn)
        {
            if (t.hist_n == cap)
                t.code_phase_rate_step_chips = hist_rate(gc->hist_code, gc->hist_samples, t.hist_head, cap,
                    c.smoother_length, slot, t.code_phase_step_chips, ns);
            gc->hist_code[slot] = t.code_phase_step_chips;
            gc->hist_samples[slot] = ns;
        }
    t.rem_code_phase_samples = K_blk - len;
    t.rem_code_phase_chips = t.code_freq_chips * t.rem_code_phase_samples / c.fs_in;
}

__device__ inline void circ_push(TrkHot& t, float2 prompt)
{
    // shift the 160-bit register left by one, new sign in at bit 0
    const uint32_t in = prompt.x < 0.0F ? 1u : 0u;
    uint32_t carry = in;
    for (int w = 0; w < 5; ++w)
        {
            const uint32_t out = t.circ[w] >> 31;
            t.circ[w] = (t.circ[w] << 1) | carry;
            carry = out;
        }
    t.circ_size++;
}

// acquire_secondary (:923-967): corr = sum over the buffer of +-1 by sign match
// = 160 - 2 * mismatches; |corr| == 160 only on a full match or full inversion.
__device__ inline int acquire_secondary(const TrkConst& c, TrkHot& t)
{
    // the last sec_len pushes sit in register bits [0, sec_len)
    int mism = 0;
    for (int w = 0; w < 5; ++w)
        {
            const int lo = w * 32;
            const uint32_t mask = c.sec_len >= lo + 32 ? 0xffffffffu : (c.sec_len > lo ? (1u << (c.sec_len - lo)) - 1u : 0u);
            mism += __popc((t.circ[w] ^ c.preamble[w]) & mask);
        }
    if (mism == 0)
        {
            t.flag_pll_180 = 0;
            return 1;
        }
    if (mism == c.sec_len)
        {
            t.flag_pll_180 = 1;
            return 1;
        }
    return 0;
}

struct EpochOut
{
    int32_t flags;
    double prompt_i, prompt_q;
    float log_accu[5];  // log_data's |VE|, |E|, |P|, |L|, |VL| accumulators (GSDR_TRK_F_LOGGED)
    bool evm;           // locked with a full prompt buffer: t.evm is wave 1's evm_of
};

// log_data (:1403-1500): the accumulator magnitudes at the reference's log point
// (std::abs<float> of the complex accumulators; VE/VL written as 0 without VEML)
__device__ inline void log_point(const TrkConst& c, const TrkHot& t, EpochOut& o)
{
    o.flags |= GSDR_TRK_F_LOGGED;
    o.log_accu[0] = c.veml ? hypotf(t.VE_accu.x, t.VE_accu.y) : 0.0F;
    o.log_accu[1] = hypotf(t.E_accu.x, t.E_accu.y);
    o.log_accu[2] = hypotf(t.P_accu.x, t.P_accu.y);
    o.log_accu[3] = hypotf(t.L_accu.x, t.L_accu.y);
    o.log_accu[4] = c.veml ? hypotf(t.VL_accu.x, t.VL_accu.y) : 0.0F;
}

// save_correlation_results (:1288-1400): secondary-code wipe-off of the tap
// accumulators, data-symbol accumulation (NH wipe-off / pilot data prompt).
// epl: the taps at c.iE / c.iP / c.iL (summed from LDS by run-time index, so no
// private array is indexed at run time)
__device__ inline void save_correlation_results(const TrkConst& c, TrkHot& t, const float2 (&taps)[kMaxTrkTaps + 1],
    const float2 (&epl)[3])
{
    float sg = 1.0F;
    if (c.secondary)
        {
            sg = ((c.sec_str[t.current_symbol >> 5] >> (t.current_symbol & 31)) & 1u) ? -1.0F : 1.0F;
            t.current_symbol++;
            t.current_symbol %= c.sec_len;
        }
    auto acc = [](float2& a, float2 b, float g) {
        if (g > 0)
            {
                a.x += b.x;
                a.y += b.y;
            }
        else
            {
                a.x -= b.x;
                a.y -= b.y;
            }
    };
    if (c.veml)
        {
            acc(t.VE_accu, taps[0], sg);
            acc(t.VL_accu, taps[4], sg);
        }
    acc(t.E_accu, epl[0], sg);
    acc(t.P_accu, epl[1], sg);
    acc(t.L_accu, epl[2], sg);
    const float2 pd = c.track_pilot ? taps[kMaxTrkTaps] : epl[1];
    if (c.symbols_per_bit > 1)
        {
            if (c.data_sec_len > 0)
                {
                    acc(t.P_data_accu, pd, ((c.data_sec_str >> t.current_data_symbol) & 1u) ? -1.0F : 1.0F);
                    t.current_data_symbol++;
                    t.current_data_symbol %= c.data_sec_len;
                }
            else
                {
                    acc(t.P_data_accu, pd, 1.0F);
                    t.current_data_symbol++;
                    t.current_data_symbol %= c.symbols_per_bit;
                }
        }
    else
        t.P_data_accu = pd;
    t.cloop = c.track_pilot ? 0 : 1;
}

// One general_work call after the correlation (taps given; slot kMaxTrkTaps is
// the pilot-tracking data prompt): states 2 and 4.
// GSDR_TRK_TIMING: wall-clock probes inside the loop update (slots 4-6 of the record)
__device__ __forceinline__ void tprobe(bool on, uint64_t (&pr)[3], int i)
{
    if (on) pr[i] = wall_clock64();
}

// run_dll_pll of a call computed speculatively (states 2 and 4) as its two halves:
// the carrier loop on wave 1, the code loop on wave 3 (into the code loop filter slot
// that is not current).  The discriminators and loop filters read nothing the CN0
// estimator and lock detector (wave 2) write, so each wave runs on its own copy of
// the state; wave 0 takes the results when the call stays locked (and drops them on a
// loss of lock).  Same operations on the same values: the loop is bit-identical to
// run_dll_pll on one wave (round 6: C2 call 6.2 -> 5.6 us, C5 GPS 10.8 -> 10.1 us,
// profiles/r06k3; with the next call's plan on wave 1 C5 GPS 9.9 us, profiles/r06p).
struct DllPllSpec  // wave 1's carrier loop of a call
{
    double carrier_doppler_hz;
    float2 P_accu_old;
    float cf_w, cf_x;
    float log_err[2];
};

// cn0_and_tracking_lock_status of a call computed by wave 2 (states 2 and 4): the
// fields it writes are disjoint from everything run_dll_pll, update_tracking_vars and
// the state transitions read or write, so wave 0 runs the locked branch without it and
// takes these results afterwards; on a loss of lock (rare) it rebuilds the call from
// the state at the call's start (s_t) exactly as the reference's early return leaves it.
struct Cn0Spec
{
    double cn0_db_hz, carrier_lock_test;
    float sm_old[2], sm_sum[2];
    int32_t sm_counter[2], sm_init[2];
    int32_t cn0_estimation_counter, carrier_lock_fail_counter, code_lock_fail_counter, locked;
};

__device__ __forceinline__ void cn0_publish(Cn0Spec& r, const TrkHot& t, int locked)
{
    r.cn0_db_hz = t.cn0_db_hz;
    r.carrier_lock_test = t.carrier_lock_test;
    for (int w = 0; w < 2; ++w)
        {
            r.sm_old[w] = t.sm_old[w];
            r.sm_sum[w] = t.sm_sum[w];
            r.sm_counter[w] = t.sm_counter[w];
            r.sm_init[w] = t.sm_init[w];
        }
    r.cn0_estimation_counter = t.cn0_estimation_counter;
    r.carrier_lock_fail_counter = t.carrier_lock_fail_counter;
    r.code_lock_fail_counter = t.code_lock_fail_counter;
    r.locked = locked;
}

__device__ __forceinline__ void cn0_apply(TrkHot& t, const Cn0Spec& r)
{
    t.cn0_db_hz = r.cn0_db_hz;
    t.carrier_lock_test = r.carrier_lock_test;
    for (int w = 0; w < 2; ++w)
        {
            t.sm_old[w] = r.sm_old[w];
            t.sm_sum[w] = r.sm_sum[w];
            t.sm_counter[w] = r.sm_counter[w];
            t.sm_init[w] = r.sm_init[w];
        }
    t.cn0_estimation_counter = r.cn0_estimation_counter;
    t.carrier_lock_fail_counter = r.carrier_lock_fail_counter;
    t.code_lock_fail_counter = r.code_lock_fail_counter;
}

struct DllSpec  // wave 3's code loop of a call
{
    double code_freq_base;  // c.code_chip_rate - the filtered code error
    float log_err2, log_err3;
};

struct SpecLink
{
    DllPllSpec* res;   // LDS
    DllSpec* dres;     // LDS
    int* dready;       // LDS: the call index whose code loop dres holds
    int* ready;        // LDS: the call index whose results res holds
    LoopFilter* lfs;   // LDS: the code loop filter's two slots
    int* lfi_lds;      // LDS: the current slot (read by wave 3 at the start of a call)
    int lfi;           // wave 0: the current slot
    int e;             // wave 0: this call's index
};

__device__ inline void take_dll_pll(const TrkConst& c, TrkHot& t, SpecLink& sl)
{
    while (__hip_atomic_load(sl.ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != sl.e)
        __builtin_amdgcn_s_sleep(1);
    const DllPllSpec r = *sl.res;
    t.carrier_doppler_hz = r.carrier_doppler_hz;
    t.P_accu_old = r.P_accu_old;
    t.cf_w = r.cf_w;
    t.cf_x = r.cf_x;
    t.log_err[0] = r.log_err[0];
    t.log_err[1] = r.log_err[1];
    while (__hip_atomic_load(sl.dready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != sl.e)
        __builtin_amdgcn_s_sleep(1);
    const DllSpec d = *sl.dres;
    t.code_freq_chips = d.code_freq_base;
    t.log_err[2] = d.log_err2;
    t.log_err[3] = d.log_err3;
    if (c.carrier_aiding) t.code_freq_chips += t.carrier_doppler_hz * c.code_chip_rate / c.signal_carrier_freq;
    sl.lfi ^= 1;  // wave 3 filtered into the other slot
}

// The call's accumulators before the lock test (states 2 and 4, :1828-1845 / :2032):
// shared by wave 2's lock test, wave 0's locked branch and its rebuild after a loss
__device__ __forceinline__ void pre_lock(const TrkConst& c, TrkHot& t, const float2 (&taps)[kMaxTrkTaps + 1],
    const float2 (&epl)[3], uint64_t nitems_read)
{
    if (t.state == 2)
        {
            if (c.veml)
                {
                    t.VE_accu = taps[0];
                    t.VL_accu = taps[4];
                }
            t.E_accu = epl[0];
            t.P_accu = epl[1];
            t.L_accu = epl[2];
            t.spc = c.early_late_space_chips;
            if (nitems_read < c.acq_sample_stamp || nitems_read - c.acq_sample_stamp >= c.bit_sync_span)
                t.carrier_lock_fail_counter = 300000;
        }
    else
        save_correlation_results(c, t, taps, epl);
}

__device__ __forceinline__ void init_out(EpochOut& o)
{
    o.flags = 0;
    o.evm = false;
    o.prompt_i = 0.0;
    o.prompt_q = 0.0;
    for (int i = 0; i < 5; ++i) o.log_accu[i] = 0.0F;
}

// States 2 and 4 run the branch of a call that stays locked; the lock test's results
// come from wave 2 (Cn0Spec) and the caller undoes the branch on a loss of lock.
// KF: the state machine of kf_tracking::general_work (kf_tracking.cc:1833-2066), which is
// this one with run_Kf in run_dll_pll's place, its own update_tracking_vars and
// update_kf_narrow_integration_time where the DLL/PLL block narrows its loop filters
template <bool KF = false, typename Link = SpecLink>
__device__ inline void after_correlation(const TrkConst& c, TrkHot& t, TrkChan* gc, Link& sl,
    const float2 (&taps)[kMaxTrkTaps + 1], const float2 (&epl)[3], uint64_t nitems_read, EpochOut& o, bool tm,
    uint64_t (&pr)[3])
{
    init_out(o);
    if (t.state == 2)
        {
            pre_lock(c, t, taps, epl, nitems_read);
            tprobe(tm, pr, 0);
                {
                    int next_state = 0;
                    if constexpr (KF)
                        take_kf(c, t, sl);
                    else
                        take_dll_pll(c, t, sl);
                    tprobe(tm, pr, 1);
                    update_tracking_vars<KF>(c, t, gc);
                    tprobe(tm, pr, 2);
                    log_point(c, t, o);
                    if (!t.pull_in_transitory)
                        {
                            if (c.secondary || c.symbols_per_bit > 1)
                                {
                                    circ_push(t, epl[1]);
                                    if (t.circ_size >= c.sec_len) next_state = acquire_secondary(c, t);
                                }
                            else
                                next_state = 1;
                        }
                    if (next_state)
                        {
                            t.VE_accu = t.E_accu = t.P_accu = t.L_accu = t.VL_accu = t.P_data_accu = make_float2(0.f, 0.f);
                            t.circ_size = 0;
                            for (int w = 0; w < 5; ++w) t.circ[w] = 0u;
                            t.current_symbol = 0;
                            t.current_data_symbol = 0;
                            o.flags |= GSDR_TRK_F_BIT_SYNC;
                            if (c.enable_ext)
                                {
                                    // extended correlator: narrow loops and taps (:1945-1983)
                                    t.extend_count = 0;
                                    if constexpr (KF)
                                        {
                                            const double Ti_old = t.corr_time;
                                            t.corr_time = c.corr_time_ext;
                                            t.state = 3;
                                            kf_narrow(c, t, sl, Ti_old, (int)(threadIdx.x & 63));
                                        }
                                    else
                                        {
                                            t.corr_time = c.corr_time_ext;
                                            t.state = 3;
                                            LoopFilter& lf = sl.lfs[sl.lfi];
                                            lf.T = (float)t.corr_time;
                                            lf_update(lf);
                                            lf.bw = c.dll_bw_narrow_hz;
                                            lf_update(lf);
                                        }
                                    t.narrow = 1;
                                    t.spc = c.early_late_space_narrow_chips;
                                }
                            else
                                t.state = 4;
                        }
                }
        }
    else if (t.state == 3)  // coherent integration (:1989-2026)
        {
            save_correlation_results(c, t, taps, epl);
            update_tracking_vars<KF>(c, t, gc);
            if (t.current_data_symbol == 0)
                {
                    log_point(c, t, o);
                    o.prompt_i = (double)(c.interchange_iq ? t.P_data_accu.y : t.P_data_accu.x);  // :2001-2010
                    o.prompt_q = (double)(c.interchange_iq ? t.P_data_accu.x : t.P_data_accu.y);
                    o.flags |= GSDR_TRK_F_VALID_OUTPUT;
                    t.P_data_accu = make_float2(0.f, 0.f);
                }
            t.extend_count++;
            if (t.extend_count == c.extend_correlation_symbols - 1)
                {
                    t.extend_count = 0;
                    t.state = 4;
                }
        }
    else  // state 4
        {
            pre_lock(c, t, taps, epl, nitems_read);
            tprobe(tm, pr, 0);
                {
                    if constexpr (KF)
                        take_kf(c, t, sl);
                    else
                        take_dll_pll(c, t, sl);
                    tprobe(tm, pr, 1);
                    update_tracking_vars<KF>(c, t, gc);
                    tprobe(tm, pr, 2);
                    if (!t.acc_carrier_phase_initialized)
                        {
                            t.acc_carrier_phase_rad = -(double)t.rem_carr_phase_rad;
                            t.acc_carrier_phase_initialized = 1;
                        }
                    if (t.current_data_symbol == 0)
                        {
                            log_point(c, t, o);
                            o.prompt_i = (double)(c.interchange_iq ? t.P_data_accu.y : t.P_data_accu.x);  // :2054-2063
                            o.prompt_q = (double)(c.interchange_iq ? t.P_data_accu.x : t.P_data_accu.y);
                            o.flags |= GSDR_TRK_F_VALID_OUTPUT;
                            t.P_data_accu = make_float2(0.f, 0.f);
                        }
                    t.VE_accu = t.E_accu = t.P_accu = t.L_accu = t.VL_accu = make_float2(0.f, 0.f);
                    if (c.enable_ext) t.state = 3;
                }
        }
    if (t.flag_pll_180) o.flags |= GSDR_TRK_F_PLL_180;
}

}  // namespace
