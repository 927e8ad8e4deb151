// Tracking: the host unit -- signal tables and channel set-up (the constructor and
// start_tracking of dll_pll_veml_tracking.cc / kf_tracking.cc), the launch plan, the
// handle and the gsdr_trk_* C ABI.  The kernel is trk_kernel.h, compiled in
// trk_dll_pll.hip and trk_kf.hip; this unit takes its instances through their getters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "gsdr_internal.h"
#include "gsdr_stream_internal.h"
#include "trk_types.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

using namespace gsdr::trk;

namespace
{

// GPS_L1_CA.h:34-73
constexpr double kGpsL1Hz = 1.57542e9;
constexpr double kGpsCaRate = 1.023e6;
constexpr double kGpsCaPeriod = 0.001;
constexpr int kGpsCaLength = 1023;
constexpr int kGpsCaSymbolsPerBit = 20;
// Galileo_E1.h:32-52
constexpr double kGalE1Hz = 1.57542e9;
constexpr double kGalE1Rate = 1.023e6;
constexpr double kGalE1Period = 0.004;
constexpr int kGalE1Length = 4092;
constexpr const char* kGalE1cSecondary = "0011100000001010110110010";
// Beidou_B1I.h:30-48
constexpr double kBdsB1Hz = 1.561098e9;
constexpr double kBdsB1Rate = 2.046e6;
constexpr double kBdsB1Period = 0.001;
constexpr int kBdsB1Length = 2046;
constexpr const char* kBdsB1Nh = "00000100110101001110";
constexpr const char* kBdsB1GeoPreamble = "1111110000001100001100";
// Galileo E5a (Galileo_E5a.h:30-39, :3581) and GPS L5 (GPS_L5.h:30-45, :167-172)
constexpr double kGalE5aHz = 1.17645e9;
constexpr double kGalE5aRate = 1.023e7;
constexpr double kGalE5aPeriod = 0.001;
constexpr int kGalE5aLength = 10230;
constexpr const char* kGalE5aISecondary = "10000100001011101001";
constexpr int kGalE5aQSecondaryLength = 100;
constexpr double kGpsL5Hz = 1.17645e9;
constexpr double kGpsL5Rate = 1.023e7;
constexpr double kGpsL5Period = 0.001;
constexpr int kGpsL5Length = 10230;
constexpr const char* kGpsL5iNh = "0000110101";
constexpr const char* kGpsL5qNh = "00000100110101001110";
constexpr const char* kGpsCaPreamble =
    "1111111111111111111100000000000000000000000000000000000000000000000000000000000011111111111111111111000000000000"
    "000000001111111111111111111111111111111111111111";
// GPS_CA_PREAMBLE_SYMBOLS_STR as a 160-bit register, string index i at bit
// (159 - i) of the 5-word big register (word 4 = most significant)
// '1' -> 1; built on the host by preamble_register().

// A secondary code / preamble string as the register acquire_secondary compares
// with: the register holds the signs of the last pushes (1 = real < 0), newest at
// bit 0, so string index i (oldest first) sits at bit len-1-i; a match for
// real < 0 is character '0' (:923-967), so the register bit is 1 where the
// character is '0'.  str_bits: bit i = (string[i] == '1').
void code_registers(const char* str, int len, uint32_t reg[5], uint32_t str_bits[5])
{
    for (int w = 0; w < 5; ++w) reg[w] = str_bits[w] = 0u;
    for (int i = 0; i < len; ++i)
        {
            const int bit = len - 1 - i;
            if (str[i] == '0') reg[bit >> 5] |= 1u << (bit & 31);
            if (str[i] == '1') str_bits[i >> 5] |= 1u << (i & 31);
        }
}

void set_secondary(TrkConst& c, const char* str, int len)
{
    c.sec_len = len;
    code_registers(str, len, c.preamble, c.sec_str);
}

}  // namespace

struct gsdr_trk
{
    int device{0};
    gsdr_trk_conf conf{};
    hipStream_t stream{nullptr};
    std::vector<TrkConst> h_consts;
    std::vector<TrkChan> h_chans;
    TrkConst* d_consts{nullptr};
    TrkChan* d_chans{nullptr};
    TrkChan* d_snap[2]{nullptr, nullptr};
    std::vector<float*> code_bufs;
    float** d_codes{nullptr};
    std::vector<float*> data_code_bufs;  // pilot tracking: data-component replicas
    float** d_data_codes{nullptr};
    std::vector<int> data_code_len;
    // per-channel pilot secondary code (gsdr_trk_set_secondary_code: Galileo E5a-Q)
    std::vector<std::string> sec_codes;
    // compact replicas: asked for (5X / L5 pilot handles, GSDR_TRK_PACK_REPLICAS=1), whether each
    // channel's two replicas are exact in f16, and whether the launches use the compact kernel
    bool pack_wanted{false};
    std::vector<char> code_f16, data_f16;
    bool pack{false};
    // Kalman loop (gsdr_trk_set_kf): the handle launches the KF kernel instance; allowed
    // until the first gsdr_trk_start
    bool kf{false};
    bool started{false};
    gsdr_trk_kf_conf kf_conf{};
    gsdr_trk_epoch* d_out{nullptr};
    uint32_t* d_nout{nullptr};
    uint32_t out_cap{0};
    void* d_iq{nullptr};
    uint64_t iq_cap{0};
    size_t lds_bytes{0};
    int code_pad{1024 + 2 * kCodeMargin};  // floats reserved for the padded replica ahead of the LDS window
    int data_pad{0};     // floats reserved for the data replica (pilot tracking)
    // GSDR_TRK_TIMING=1: per-phase clock64 stamps of every call, summarised on destroy
    bool timing_on{false};
    int timing_wall{0};  // GSDR_TRK_TIMING=2: constant-rate wall clock instead of the shader clock
    uint64_t* d_timing{nullptr};
    size_t timing_cap{0};
    double tsum[kTimingSlots]{};
    uint32_t timing_epochs{0};
    uint32_t* timing_nout{nullptr};
    uint64_t tcount{0};
    bool profiling{false};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    // recorded after every launch on the stream it used: host read-modify-writes of
    // d_chans (start / stop / get_channel) wait for it, so a launch in flight on a
    // caller stream cannot write a stale channel back over them
    hipEvent_t last_launch{nullptr};
    // gsdr_trk_submit_stream / gsdr_trk_collect: device records of the submission,
    // their pinned host image and the event of its copy
    struct Submission
    {
        // the kernel writes the records straight into pinned host memory (zero-copy):
        // no copy-engine hop between one advance's kernel and the next on the stream
        gsdr_trk_epoch* h_out{nullptr};
        uint32_t* h_nout{nullptr};
        uint32_t cap{0};  // records per channel the buffers hold
        uint32_t epochs{0};
        hipEvent_t done{nullptr};
    };
    static constexpr int kSubmissions = 2;  // in flight at once (collected oldest first)
    Submission sub[kSubmissions];
    int sub_head{0};   // the oldest pending submission
    int sub_count{0};  // pending submissions
    std::mutex mu;
    // held for a whole gsdr_trk_submit_stream: the slot it picks stays its own while
    // mu is released for the launch (a second submitter waits; a collect in between
    // takes only committed submissions and leaves sub_head + sub_count unchanged)
    std::mutex submit_mu;
};

namespace
{

// constructor (dll_pll_veml_tracking.cc:85-560) for one channel slot, GPS L1 C/A
// Tracking_FLL_PLL_filter::set_params (tracking_FLL_PLL_filter.cc:23-58)
void cf_set_params(CfConst& p, float fll_bw, float pll_bw, int order)
{
    p = CfConst{};
    p.order = order;
    if (order == 3)
        {
            p.b3 = 2.400F;
            p.a3 = 1.100F;
            p.a2 = 1.414F;
            p.w0p = pll_bw / 0.7845F;
            p.w0p2 = p.w0p * p.w0p;
            p.w0p3 = p.w0p2 * p.w0p;
            p.w0f = fll_bw / 0.53F;
            p.w0f2 = p.w0f * p.w0f;
        }
    else
        {
            p.a2 = 1.414F;
            p.w0p = pll_bw / 0.53F;
            p.w0p2 = p.w0p * p.w0p;
            p.w0f = fll_bw / 0.25F;
        }
}

// Exponential_Smoother::set_alpha (exponential_smoother.cc:29-41)
void sm_set(SmConst& k, float alpha, float min_value, float offset, int samples)
{
    k.alpha = alpha;
    if (k.alpha < 0) k.alpha = 0;
    if (k.alpha > 1) k.alpha = 1;
    k.one_minus_alpha = 1.0F - k.alpha;
    k.min_value = min_value;
    k.offset = offset;
    k.samples_init = std::max(1, samples);
}

// tap shifts (:466-507 / :850-862), in replica samples; the narrow set of the
// extended correlator (:1963-1977)
void set_shifts(const gsdr_trk_conf& cf, TrkConst& c)
{
    const float spc = (float)c.code_samples_per_chip;
    if (c.veml)
        {
            c.shifts[0] = -cf.very_early_late_space_chips * spc;
            c.shifts[1] = -cf.early_late_space_chips * spc;
            c.shifts[2] = 0.0F;
            c.shifts[3] = cf.early_late_space_chips * spc;
            c.shifts[4] = cf.very_early_late_space_chips * spc;
            c.shifts_narrow[0] = -cf.very_early_late_space_narrow_chips * spc;
            c.shifts_narrow[1] = -cf.early_late_space_narrow_chips * spc;
            c.shifts_narrow[2] = 0.0F;
            c.shifts_narrow[3] = cf.early_late_space_narrow_chips * spc;
            c.shifts_narrow[4] = cf.very_early_late_space_narrow_chips * spc;
        }
    else
        {
            c.shifts[0] = -cf.early_late_space_chips * spc;
            c.shifts[1] = 0.0F;
            c.shifts[2] = cf.early_late_space_chips * spc;
            c.shifts_narrow[0] = -cf.early_late_space_narrow_chips * spc;
            c.shifts_narrow[1] = 0.0F;
            c.shifts_narrow[2] = cf.early_late_space_narrow_chips * spc;
        }
}

// signal table of the constructor (dll_pll_veml_tracking.cc:170-430)
struct SignalParams
{
    double carrier_hz, period_s, chip_rate;
    int length_chips, samples_per_chip, symbols_per_bit, veml;
};
SignalParams signal_params(int signal)
{
    if (signal == GSDR_SIGNAL_GAL_1B) return {kGalE1Hz, kGalE1Period, kGalE1Rate, kGalE1Length, 2, 1, 1};
    if (signal == GSDR_SIGNAL_BDS_B1) return {kBdsB1Hz, kBdsB1Period, kBdsB1Rate, kBdsB1Length, 1, 20, 0};
    if (signal == GSDR_SIGNAL_GAL_5X) return {kGalE5aHz, kGalE5aPeriod, kGalE5aRate, kGalE5aLength, 1, 20, 0};  // :289-319
    if (signal == GSDR_SIGNAL_GPS_L5) return {kGpsL5Hz, kGpsL5Period, kGpsL5Rate, kGpsL5Length, 1, 10, 0};      // :210-244
    return {kGpsL1Hz, kGpsCaPeriod, kGpsCaRate, kGpsCaLength, 1, kGpsCaSymbolsPerBit, 0};
}

// constructor (dll_pll_veml_tracking.cc:85-560) for one channel slot
void init_channel(const gsdr_trk_conf& cf, TrkConst& c, TrkChan& ch)
{
    std::memset(&c, 0, sizeof(c));
    std::memset(&ch, 0, sizeof(ch));
    const SignalParams sp = signal_params(cf.signal);
    c.fs_in = cf.fs_in;
    c.code_period = sp.period_s;
    c.code_chip_rate = sp.chip_rate;
    c.signal_carrier_freq = sp.carrier_hz;
    c.veml = sp.veml;
    c.iE = c.veml ? 1 : 0;
    c.iP = c.veml ? 2 : 1;
    c.iL = c.veml ? 3 : 2;
    if (cf.signal == GSDR_SIGNAL_GAL_1B)
        {
            c.track_pilot = cf.track_pilot ? 1 : 0;
            c.secondary = c.track_pilot;
            if (c.secondary) set_secondary(c, kGalE1cSecondary, 25);
        }
    else if (cf.signal == GSDR_SIGNAL_BDS_B1)
        {
            // D1 by default; gsdr_trk_start switches GEO PRNs to the D2 preamble
            c.secondary = 1;
            set_secondary(c, kBdsB1Nh, 20);
            uint32_t reg[5], bits[5];
            code_registers(kBdsB1Nh, 20, reg, bits);
            c.data_sec_len = 20;
            c.data_sec_str = bits[0];
        }
    else if (cf.signal == GSDR_SIGNAL_GAL_5X)
        {
            c.track_pilot = cf.track_pilot ? 1 : 0;
            c.secondary = 1;
            uint32_t reg[5], bits[5];
            code_registers(kGalE5aISecondary, 20, reg, bits);
            if (c.track_pilot)
                {
                    // the E5a-Q secondary code is the PRN's (gsdr_trk_start, :703); the
                    // E5a-I one is wiped from the data prompt (:306-310)
                    c.sec_len = kGalE5aQSecondaryLength;
                    c.data_sec_len = 20;
                    c.data_sec_str = bits[0];
                    c.interchange_iq = 1;
                }
            else
                set_secondary(c, kGalE5aISecondary, 20);  // d_data_secondary_code_length stays 0 (:312-317)
        }
    else if (cf.signal == GSDR_SIGNAL_GPS_L5)
        {
            c.track_pilot = cf.track_pilot ? 1 : 0;
            c.secondary = 1;
            if (c.track_pilot)
                {
                    set_secondary(c, kGpsL5qNh, 20);  // :224-234
                    uint32_t reg[5], bits[5];
                    code_registers(kGpsL5iNh, 10, reg, bits);
                    c.data_sec_len = 10;
                    c.data_sec_str = bits[0];
                }
            else
                {
                    set_secondary(c, kGpsL5iNh, 10);  // :236-243
                    c.interchange_iq = 1;
                }
        }
    else
        set_secondary(c, kGpsCaPreamble, kPreambleLen);
    c.carrier_lock_threshold = cf.carrier_lock_th;
    c.early_late_space_chips = cf.early_late_space_chips;
    c.vector_length = (int32_t)cf.vector_length;
    c.code_length_chips = sp.length_chips;
    c.code_samples_per_chip = sp.samples_per_chip;
    c.symbols_per_bit = sp.symbols_per_bit;
    c.cn0_samples = cf.cn0_samples;
    c.cn0_min = cf.cn0_min;
    c.max_code_lock_fail = cf.max_code_lock_fail;
    c.max_carrier_lock_fail = cf.max_carrier_lock_fail;
    const uint64_t fsi = (uint64_t)(int64_t)(int)cf.fs_in;
    c.pull_in_span = ((uint64_t)cf.pull_in_time_s + 1) * fsi;
    c.bit_sync_span = ((uint64_t)cf.bit_synchronization_time_limit_s + 1) * fsi;
    c.extend_correlation_symbols = cf.extend_correlation_symbols;
    c.enable_fll_pull_in = cf.enable_fll_pull_in;
    c.enable_fll_steady_state = cf.enable_fll_steady_state;
    c.carrier_aiding = cf.carrier_aiding;
    c.n_taps = c.veml ? 5 : 3;
    set_shifts(cf, c);
    cf_set_params(c.cf, cf.fll_bw_hz, cf.pll_bw_hz, cf.pll_filter_order);
    cf_set_params(c.cf_narrow, cf.fll_bw_hz, cf.pll_bw_narrow_hz, cf.pll_filter_order);
    c.early_late_space_narrow_chips = cf.early_late_space_narrow_chips;
    c.dll_bw_narrow_hz = cf.dll_bw_narrow_hz;
    c.enable_ext = cf.extend_correlation_symbols > 1 ? 1 : 0;
    c.high_dyn = cf.high_dyn ? 1 : 0;
    // dll_pll_conf.cc:118-123: smoother_length < 1 is set to 1
    c.smoother_length = cf.smoother_length < 1 ? 1 : (int32_t)cf.smoother_length;
    c.kf_beta = c.code_chip_rate / c.signal_carrier_freq;
    // Exponential_Smoother defaults (exponential_smoother.h:58-63) + dll_pll_veml_tracking.cc:540-552
    sm_set(c.sm[0], cf.cn0_smoother_alpha, 25.0F, 12.0F, cf.cn0_smoother_samples / (int)(c.code_period * 1000.0));
    sm_set(c.sm[1], cf.carrier_lock_test_smoother_alpha, -1.0F, 0.0F, cf.carrier_lock_test_smoother_samples);
    TrkHot& t = ch.h;
    t.spc = cf.early_late_space_chips;
    t.code_freq_chips = c.code_chip_rate;
    t.corr_time = c.code_period;
    sm_reset(t, 0);
    sm_reset(t, 1);
    t.state = 0;
    ch.code_filter.T = (float)c.code_period;
    ch.code_filter.bw = cf.dll_bw_hz;
    ch.code_filter.order = cf.dll_filter_order;
    lf_update(ch.code_filter);
}

int ensure_out(gsdr_trk* k, uint32_t max_epochs)
{
    const uint64_t need = (uint64_t)k->conf.max_channels * max_epochs;
    if (need <= k->out_cap) return GSDR_OK;
    if (k->d_out) GSDR_HIP(hipFree(k->d_out));
    k->d_out = nullptr;
    k->out_cap = 0;
    GSDR_HIP(hipMalloc(&k->d_out, need * sizeof(gsdr_trk_epoch)));
    k->out_cap = (uint32_t)need;
    return GSDR_OK;
}

// every value survives the round trip through f16 (the compact replica's halves)
bool f16_exact(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!((float)(_Float16)v[i] == v[i])) return false;
    return true;
}

// Dynamic LDS of a launch: the replica and the input window, padded up to a whole
// CU's LDS so that no workgroup of another kernel (the acquisition grid on the
// other queue) can share the CU with a tracking workgroup -- the loop is a
// latency chain and co-resident FFT waves would slow every call down.
constexpr size_t kCuLds = 160 * 1024;
constexpr size_t kStaticLdsMargin = 4 * 1024;  // the kernel's static __shared__ arrays
// Streamed calls (vector_length > kWinCore): two chunk buffers in the LDS left
// after the replicas, each (chunk + kTrkThreads + kHalo) items (a last chunk carries
// a tail of up to kTrkThreads samples) + 16 alignment bytes rounded up to whole
// glds rows; chunk a multiple of kWinCore.  chunk = 0: no room (the
// calls then read HBM directly).
int stream_buffer_bytes(int chunk, int isz) { return (((chunk + kHalo) * isz + 16) / kStreamRow + 2) * kStreamRow; }
void stream_plan(size_t lds_bytes, int code_pad, int data_pad, int isz, int& chunk, int& sbuf)
{
    const long avail = (long)lds_bytes - (long)(code_pad + data_pad) * (long)sizeof(float);
    chunk = 0;
    sbuf = 0;
    int cap = 64 * kWinCore;
    if (const char* e = std::getenv("GSDR_TRK_STREAM_CHUNK")) cap = std::max(kWinCore, std::atoi(e) / kWinCore * kWinCore);
    for (int c = kWinCore; c <= cap; c += kWinCore)
        {
            if (2L * stream_buffer_bytes(c + kTrkThreads, isz) > avail) break;
            chunk = c;
            sbuf = stream_buffer_bytes(c + kTrkThreads, isz);
        }
}

size_t lds_for(int code_pad, int data_pad)
{
    const size_t need = (size_t)(code_pad + data_pad) * sizeof(float) +
                        std::max((size_t)(kWinCore + kHalo) * sizeof(float2), (size_t)2 * stream_buffer_bytes(kWinCore + kTrkThreads, 8));
    // LDS reserved per channel workgroup: by default the whole CU, so no acquisition
    // workgroup shares its issue slots once it runs; GSDR_TRK_LDS_KB trades that for
    // an earlier start on a busy chip (a full-CU workgroup waits for an empty CU).
    size_t reserve = kCuLds - kStaticLdsMargin;
    if (const char* e = std::getenv("GSDR_TRK_LDS_KB")) reserve = std::min(reserve, (size_t)std::atoi(e) * 1024);
    return std::max(need, reserve);
}

// the kernel instance of an item type, replica layout and loop
TrkKernel trk_kernel_of(int item_type, bool pack, bool kf = false)
{
    return kf ? gsdr::trk_kf_kernel(item_type, pack) : gsdr::trk_dll_pll_kernel(item_type, pack);
}

int launch(gsdr_trk* k, const void* iq, uint64_t iq_first, uint64_t iq_items, uint32_t max_epochs, gsdr_trk_epoch* out,
    uint32_t* nout, hipStream_t s)
{
    uint64_t* timing = nullptr;
    if (k->timing_on)
        {
            const size_t need = (size_t)k->conf.max_channels * max_epochs * kTimingSlots;
            if (need > k->timing_cap)
                {
                    if (k->d_timing) GSDR_HIP(hipFree(k->d_timing));
                    k->d_timing = nullptr;
                    k->timing_cap = 0;
                    GSDR_HIP(hipMalloc(&k->d_timing, need * sizeof(uint64_t)));
                    k->timing_cap = need;
                }
            timing = k->d_timing;
        }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (k->profiling)
        {
            for (hipEvent_t* e : {&e0, &e1})
                {
                    if (!k->prof_pool.empty())
                        {
                            *e = k->prof_pool.back();
                            k->prof_pool.pop_back();
                        }
                    else
                        GSDR_HIP(hipEventCreate(e));
                }
            GSDR_HIP(hipEventRecord(e0, s));
        }
    const dim3 grid(k->conf.max_channels);
    int chunk = 0, sbuf = 0;
    stream_plan(k->lds_bytes, k->code_pad, k->data_pad, (int)gsdr::item_bytes(k->conf.item_type), chunk, sbuf);
    const TrkKernel kern = trk_kernel_of(k->conf.item_type, k->pack, k->kf);
    hipLaunchKernelGGL(kern, grid, dim3(kTrkThreads), k->lds_bytes, s, k->d_consts, k->d_chans,
        (const float* const*)k->d_codes, (const float* const*)k->d_data_codes, iq, iq_first, iq_items, max_epochs, out, nout,
        k->code_pad, k->data_pad, timing, k->timing_wall, chunk, sbuf);
    GSDR_HIP(hipGetLastError());
    GSDR_HIP(hipEventRecord(k->last_launch, s));
    if (k->profiling)
        {
            GSDR_HIP(hipEventRecord(e1, s));
            k->prof_recs.push_back({e0, e1});
        }
    if (timing)
        {
            k->timing_epochs = max_epochs;  // summarised (last launch) on destroy, no sync here
            k->timing_nout = nout;
        }
    return GSDR_OK;
}

}  // namespace

extern "C" {

void gsdr_trk_conf_default(gsdr_trk_conf* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->fs_in = 2000000.0;
    c->carrier_lock_th = 0.7;
    c->signal = GSDR_SIGNAL_GPS_1C;
    c->item_type = GSDR_ITEM_GR_COMPLEX;
    c->max_channels = 1;
    c->fll_bw_hz = 35.0F;
    c->pll_bw_hz = 35.0F;
    c->dll_bw_hz = 2.0F;
    c->pll_bw_narrow_hz = 5.0F;
    c->dll_bw_narrow_hz = 0.75F;
    c->early_late_space_chips = 0.25F;
    c->very_early_late_space_chips = 0.5F;
    c->early_late_space_narrow_chips = 0.15F;
    c->very_early_late_space_narrow_chips = 0.5F;
    c->cn0_smoother_alpha = 0.002F;
    c->carrier_lock_test_smoother_alpha = 0.002F;
    c->pull_in_time_s = 10U;
    c->bit_synchronization_time_limit_s = 20U;
    c->pll_filter_order = 3;
    c->dll_filter_order = 2;
    c->extend_correlation_symbols = 1;
    c->smoother_length = 10;
    c->cn0_samples = 20;
    c->cn0_smoother_samples = 200;
    c->carrier_lock_test_smoother_samples = 25;
    c->cn0_min = 25;
    c->max_code_lock_fail = 50;
    c->max_carrier_lock_fail = 5000;
    c->carrier_aiding = 1;
}

int gsdr_trk_create(int device, const gsdr_trk_conf* conf, gsdr_trk** out)
{
    GSDR_REQUIRE(conf && out, GSDR_E_ARG, "gsdr_trk_create: null argument");
    *out = nullptr;
    GSDR_REQUIRE(conf->fs_in > 0.0, GSDR_E_ARG, "gsdr_trk_create: fs_in must be > 0");
    GSDR_REQUIRE(conf->max_channels > 0, GSDR_E_ARG, "gsdr_trk_create: max_channels must be > 0");
    GSDR_REQUIRE(conf->signal >= GSDR_SIGNAL_GPS_1C && conf->signal <= GSDR_SIGNAL_GPS_L5, GSDR_E_UNSUPPORTED,
        "gsdr_trk_create: signal %d not implemented", conf->signal);
    GSDR_REQUIRE(conf->item_type >= GSDR_ITEM_GR_COMPLEX && conf->item_type <= GSDR_ITEM_IBYTE, GSDR_E_ARG,
        "gsdr_trk_create: unknown item type %d", conf->item_type);
    GSDR_REQUIRE(conf->extend_correlation_symbols >= 1, GSDR_E_ARG,
        "gsdr_trk_create: extend_correlation_symbols must be >= 1");
    GSDR_REQUIRE(!conf->high_dyn || conf->smoother_length <= (uint32_t)kMaxSmoother, GSDR_E_UNSUPPORTED,
        "gsdr_trk_create: smoother_length %u > %d", conf->smoother_length, kMaxSmoother);
    GSDR_REQUIRE(conf->cn0_samples >= 1 && conf->cn0_samples <= kMaxCn0, GSDR_E_UNSUPPORTED,
        "gsdr_trk_create: cn0_samples %d outside [1,%d]", conf->cn0_samples, kMaxCn0);
    GSDR_REQUIRE(conf->pll_filter_order == 2 || conf->pll_filter_order == 3, GSDR_E_ARG,
        "gsdr_trk_create: pll_filter_order must be 2 or 3");
    GSDR_REQUIRE(conf->dll_filter_order >= 1 && conf->dll_filter_order <= 3, GSDR_E_ARG,
        "gsdr_trk_create: dll_filter_order must be 1..3");
    int ndev = 0;
    GSDR_HIP(hipGetDeviceCount(&ndev));
    GSDR_REQUIRE(device >= 0 && device < ndev, GSDR_E_ARG, "gsdr_trk_create: device %d of %d", device, ndev);
    gsdr::DeviceGuard g(device);
    gsdr_trk* k = new (std::nothrow) gsdr_trk();
    GSDR_REQUIRE(k, GSDR_E_ALLOC, "gsdr_trk_create: out of host memory");
    k->device = device;
    k->conf = *conf;
    // GPS L1 C/A and BeiDou B1I force track_pilot off (dll_pll_veml_tracking.cc:183, :402)
    // Galileo E1, E5a and GPS L5 honour it (:210-244, :258-319)
    if (k->conf.signal != GSDR_SIGNAL_GAL_1B && k->conf.signal != GSDR_SIGNAL_GAL_5X && k->conf.signal != GSDR_SIGNAL_GPS_L5)
        k->conf.track_pilot = 0;
    {
        const char* pe = std::getenv("GSDR_TRK_PACK_REPLICAS");
        const bool wide = k->conf.signal == GSDR_SIGNAL_GAL_5X || k->conf.signal == GSDR_SIGNAL_GPS_L5;
        k->pack_wanted = k->conf.track_pilot && !k->conf.high_dyn && (wide || (pe && std::atoi(pe) != 0));
    }
    {
        // the adapters' vector_length = round(fs_in / (chip rate / code length))
        const SignalParams sp = signal_params(k->conf.signal);
        if (k->conf.vector_length == 0)
            k->conf.vector_length = (uint32_t)std::lround(conf->fs_in / (sp.chip_rate / (double)sp.length_chips));
    }
    const uint32_t nch = k->conf.max_channels;
    k->h_consts.resize(nch);
    k->h_chans.resize(nch);
    for (uint32_t c = 0; c < nch; ++c) init_channel(k->conf, k->h_consts[c], k->h_chans[c]);
    k->code_bufs.assign(nch, nullptr);
    k->data_code_bufs.assign(nch, nullptr);
    k->data_code_len.assign(nch, 0);
    k->sec_codes.assign(nch, std::string());
    k->code_f16.assign(nch, 1);
    k->data_f16.assign(nch, 1);
    k->code_pad = 1024 + 2 * kCodeMargin;  // grows with the longest replica started (gsdr_trk_start)
    k->data_pad = 0;
    k->lds_bytes = lds_for(k->code_pad, k->data_pad);
    if (const char* tv = std::getenv("GSDR_TRK_TIMING"))
        {
            k->timing_on = std::atoi(tv) != 0;
            k->timing_wall = std::atoi(tv) == 2;
        }
    hipError_t e = hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&k->last_launch, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&k->d_consts, nch * sizeof(TrkConst));
    if (e == hipSuccess) e = hipMalloc(&k->d_chans, nch * sizeof(TrkChan));
    if (e == hipSuccess) e = hipMalloc(&k->d_snap[0], nch * sizeof(TrkChan));
    if (e == hipSuccess) e = hipMalloc(&k->d_snap[1], nch * sizeof(TrkChan));
    if (e == hipSuccess) e = hipMalloc(&k->d_codes, nch * sizeof(float*));
    if (e == hipSuccess) e = hipMalloc(&k->d_nout, nch * sizeof(uint32_t));
    for (uint32_t c = 0; c < nch && e == hipSuccess; ++c) e = hipMalloc(&k->code_bufs[c], kMaxCodeFloats * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(k->d_codes, k->code_bufs.data(), nch * sizeof(float*), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&k->d_data_codes, nch * sizeof(float*));
    if (k->conf.track_pilot)
        for (uint32_t c = 0; c < nch && e == hipSuccess; ++c)
            e = hipMalloc(&k->data_code_bufs[c], kMaxCodeFloats * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(k->d_data_codes, k->data_code_bufs.data(), nch * sizeof(float*), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(k->d_consts, k->h_consts.data(), nch * sizeof(TrkConst), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(k->d_chans, k->h_chans.data(), nch * sizeof(TrkChan), hipMemcpyHostToDevice);
    for (int it : {GSDR_ITEM_GR_COMPLEX, GSDR_ITEM_CSHORT, GSDR_ITEM_IBYTE})
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void*)trk_kernel_of(it, false), hipFuncAttributeMaxDynamicSharedMemorySize,
                (int)(kCuLds - kStaticLdsMargin));
    // and the compact instance this handle can launch beside those
    if (k->pack_wanted && e == hipSuccess)
        e = hipFuncSetAttribute((const void*)trk_kernel_of(k->conf.item_type, true),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - kStaticLdsMargin));
    if (e != hipSuccess)
        {
            gsdr::set_error("gsdr_trk_create: %s", hipGetErrorString(e));
            gsdr_trk_destroy(k);
            return GSDR_E_ALLOC;
        }
    *out = k;
    return GSDR_OK;
}

void gsdr_trk_destroy(gsdr_trk* k)
{
    if (!k) return;
    gsdr::DeviceGuard g(k->device);
    if (k->stream) (void)hipStreamSynchronize(k->stream);
    if (k->timing_on && k->d_timing && k->timing_epochs)
        {
            const uint32_t nch = k->conf.max_channels, me = k->timing_epochs;
            std::vector<uint64_t> tm((size_t)nch * me * kTimingSlots);
            std::vector<uint32_t> cnt(nch);
            if (hipMemcpy(tm.data(), k->d_timing, tm.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(cnt.data(), k->timing_nout, nch * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess)
                for (uint32_t c = 0; c < nch; ++c)
                    for (uint32_t e = 0; e < cnt[c] && e < me; ++e)
                        {
                            const uint64_t* r = &tm[((size_t)c * me + e) * kTimingSlots];
                            for (int q = 0; q + 1 < kStampSlots; ++q)
                                if (r[q + 1] >= r[q]) k->tsum[q] += (double)(r[q + 1] - r[q]);
                            if (e + 1 < cnt[c] && e + 1 < me)
                                {
                                    const uint64_t next0 = tm[((size_t)c * me + e + 1) * kTimingSlots];
                                    if (next0 >= r[kStampSlots - 1]) k->tsum[kStampSlots - 1] += (double)(next0 - r[kStampSlots - 1]);
                                }
                            for (int q = kStampSlots; q < kTimingSlots; ++q) k->tsum[q] += (double)r[q];  // durations / offsets
                            k->tcount++;
                        }
        }
    if (k->timing_on && k->tcount)
        {
            static const char* names[kTimingSlots] = {"prep", "correlate", "state-load", "tap-sum", "cn0-lock", "dll-pll",
                "update-vars", "rest", "next-plan", "loop-top", "(correlate's stream-wait)", "(w2 lock-test start)",
                "(w2 lock-test end)", "(w0 at the lock join)", "(w1 EVM end)", "(w0 at the EVM join)",
                "(w0 past the EVM join)"};
            std::fprintf(stderr, "gsdr_trk timing: %llu calls, %s ticks per call:", (unsigned long long)k->tcount,
                "wall_clock64 (100 MHz)");
            for (int q = 0; q < kTimingSlots; ++q) std::fprintf(stderr, " %s %.0f", names[q], k->tsum[q] / k->tcount);
            std::fprintf(stderr, "\n");
        }
    if (k->d_timing) (void)hipFree(k->d_timing);
    for (auto& r : k->prof_recs)
        {
            (void)hipEventDestroy(r.first);
            (void)hipEventDestroy(r.second);
        }
    for (hipEvent_t e : k->prof_pool) (void)hipEventDestroy(e);
    for (auto& u : k->sub)
        {
            if (u.done)
                {
                    (void)hipEventSynchronize(u.done);
                    (void)hipEventDestroy(u.done);
                }
            if (u.h_out) (void)hipHostFree(u.h_out);
            if (u.h_nout) (void)hipHostFree(u.h_nout);
        }
    if (k->last_launch)
        {
            (void)hipEventSynchronize(k->last_launch);
            (void)hipEventDestroy(k->last_launch);
        }
    for (float* p : k->code_bufs)
        if (p) (void)hipFree(p);
    for (float* p : k->data_code_bufs)
        if (p) (void)hipFree(p);
    void* bufs[] = {k->d_consts, k->d_chans, k->d_snap[0], k->d_snap[1], k->d_codes, k->d_data_codes, k->d_nout, k->d_out,
        k->d_iq};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (k->stream) (void)hipStreamDestroy(k->stream);
    delete k;
}

int gsdr_trk_start(gsdr_trk* k, int ch, uint32_t prn, const float* code, int code_samples, double acq_delay_samples,
    double acq_doppler_hz, uint64_t acq_samplestamp, uint64_t nitems_read, uint64_t* first_sample)
{
    GSDR_REQUIRE(k && code && first_sample, GSDR_E_ARG, "gsdr_trk_start: null argument");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_start: channel %d outside [0,%u)", ch,
        k->conf.max_channels);
    GSDR_REQUIRE(code_samples >= 1 && code_samples <= kMaxCodeFloats, GSDR_E_UNSUPPORTED,
        "gsdr_trk_start: code replica of %d samples outside [1,%d]", code_samples, kMaxCodeFloats);
    GSDR_REQUIRE(!k->conf.track_pilot || k->data_code_len[ch] == code_samples, GSDR_E_STATE,
        "gsdr_trk_start: pilot tracking needs gsdr_trk_set_data_code with %d samples for channel %d first", code_samples,
        ch);
    const bool e5a_pilot = k->conf.signal == GSDR_SIGNAL_GAL_5X && k->conf.track_pilot;
    GSDR_REQUIRE(!e5a_pilot || !k->sec_codes[ch].empty(), GSDR_E_STATE,
        "gsdr_trk_start: E5a pilot tracking needs gsdr_trk_set_secondary_code for channel %d first", ch);
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    // the device copy is authoritative between launches (the loop runs there)
    GSDR_HIP(hipStreamWaitEvent(k->stream, k->last_launch, 0));
    GSDR_HIP(hipMemcpyAsync(&k->h_chans[ch], k->d_chans + ch, sizeof(TrkChan), hipMemcpyDeviceToHost, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    TrkConst& c = k->h_consts[ch];
    TrkChan& tc = k->h_chans[ch];
    TrkHot& t = tc.h;
    // start_tracking (:640-882)
    c.prn = prn;
    if (k->conf.signal == GSDR_SIGNAL_BDS_B1)
        {
            uint32_t reg[5], bits[5];
            if ((prn > 0 && prn < 6) || prn > 58)
                {
                    // GEO (D2): D2 preamble search, 2 symbols per bit (:762-778)
                    c.symbols_per_bit = 2;
                    c.secondary = 0;
                    set_secondary(c, kBdsB1GeoPreamble, 22);
                    c.data_sec_len = 0;
                    c.data_sec_str = 0;
                }
            else
                {
                    // D1: NH code, wiped from the data symbols too (:779-795)
                    c.symbols_per_bit = 20;
                    c.secondary = 1;
                    set_secondary(c, kBdsB1Nh, 20);
                    code_registers(kBdsB1Nh, 20, reg, bits);
                    c.data_sec_len = 20;
                    c.data_sec_str = bits[0];
                }
        }
    // d_secondary_code_string = GALILEO_E5A_Q_SECONDARY_CODE[PRN - 1] (:703), here the caller's
    if (e5a_pilot) set_secondary(c, k->sec_codes[ch].data(), (int)k->sec_codes[ch].size());
    c.code_samples = code_samples;
    c.acq_sample_stamp = acq_samplestamp;
    double acq_code_phase_samples = acq_delay_samples;
    t.carrier_doppler_hz = acq_doppler_hz;
    t.carrier_phase_step_rad = kTwoPi * t.carrier_doppler_hz / c.fs_in;
    t.carrier_phase_rate_step_rad = 0.0;
    t.hist_n = 0;  // d_carr_ph_history.clear(), d_code_ph_history.clear() (:651-652)
    t.hist_head = 0;
    t.carrier_lock_fail_counter = 0;
    t.code_lock_fail_counter = 0;
    t.rem_code_phase_samples = 0.0;
    t.rem_carr_phase_rad = 0.0F;
    t.rem_code_phase_chips = 0.0;
    t.acc_carrier_phase_rad = 0.0;
    t.cn0_estimation_counter = 0;
    t.carrier_lock_test = 1.0;
    t.cn0_db_hz = 0.0;
    t.evm = 0.0;
    set_shifts(k->conf, c);
    t.corr_time = c.code_period;  // :860
    t.narrow = 0;
    t.extend_count = 0;
    c.extend_correlation_symbols = std::max(1, k->conf.extend_correlation_symbols);  // :657
    if (k->conf.signal == GSDR_SIGNAL_BDS_B1 && ((prn > 0 && prn < 6) || prn > 58))
        c.extend_correlation_symbols = std::min(c.extend_correlation_symbols, 2);  // GEO (:775-778)
    c.corr_time_ext = (double)((float)c.extend_correlation_symbols * (float)c.code_period);  // :1949
    cf_set_params(c.cf, k->conf.fll_bw_hz, k->conf.pll_bw_hz, k->conf.pll_filter_order);
    tc.code_filter.bw = k->conf.dll_bw_hz;
    lf_update(tc.code_filter);
    tc.code_filter.T = (float)c.code_period;
    lf_update(tc.code_filter);
    // Tracking_FLL_PLL_filter::initialize (tracking_FLL_PLL_filter.cc:61-74)
    const float dop0 = (float)acq_doppler_hz;
    if (c.cf.order == 3)
        {
            t.cf_x = 2.0F * dop0;
            t.cf_w = 0;
        }
    else
        {
            t.cf_w = dop0;
            t.cf_x = 0;
        }
    lf_initialize(tc.code_filter, 0.0F);
    t.cloop = 1;
    t.pull_in_transitory = 1;
    t.circ_size = 0;
    for (int w = 0; w < 5; ++w) t.circ[w] = 0u;
    t.acc_carrier_phase_initialized = 0;
    // state 1: pull-in alignment (:1813-1844)
    const int64_t diff = (int64_t)nitems_read - (int64_t)c.acq_sample_stamp;
    const double delta = (double)diff - acq_code_phase_samples;
    t.code_freq_chips = c.code_chip_rate;
    t.code_phase_step_chips = t.code_freq_chips / c.fs_in;
    t.code_phase_rate_step_chips = 0.0;
    const double T_chip_mod = 1.0 / t.code_freq_chips;
    const double T_prn_mod = T_chip_mod * (double)c.code_length_chips;
    const double T_prn_mod_samples = T_prn_mod * c.fs_in;
    acq_code_phase_samples = T_prn_mod_samples - std::fmod(delta, T_prn_mod_samples);
    t.current_prn_length_samples = (int32_t)std::round(T_prn_mod_samples);
    const int32_t offset = (int32_t)std::round(acq_code_phase_samples);
    t.acc_carrier_phase_rad -= t.carrier_phase_step_rad * (double)offset;
    t.state = 2;
    sm_reset(t, 0);
    sm_reset(t, 1);
    t.next_sample = nitems_read + (uint64_t)(int64_t)offset;
    *first_sample = t.next_sample;
    if (k->kf)
        {
            // init_kf(0.0, d_carrier_doppler_kf_hz) of the pull-in call (kf_tracking.cc:1824,
            // :857-895); d_F and d_H follow t.corr_time
            const gsdr_trk_kf_conf& q = k->kf_conf;
            TrkKf& f = tc.kf;
            std::memset(&f, 0, sizeof(f));
            f.R[0] = std::pow(q.code_disc_sd_chips, 2.0);
            f.R[1] = std::pow(q.carrier_disc_sd_rads, 2.0);
            const double qd[4] = {q.code_phase_sd_chips, q.carrier_phase_sd_rad, q.carrier_freq_sd_hz, q.carrier_freq_rate_sd_hz_s};
            const double pd[4] = {q.init_code_phase_sd_chips, q.init_carrier_phase_sd_rad, q.init_carrier_freq_sd_hz,
                q.init_carrier_freq_rate_sd_hz_s};
            for (int i = 0; i < 4; ++i)
                {
                    f.Q[5 * i] = std::pow(qd[i], 2.0);
                    f.P[5 * i] = std::pow(pd[i], 2.0);
                }
            f.x[2] = acq_doppler_hz;
        }
    {
        const int cp = std::max(k->code_pad, (code_samples + 2 * kCodeMargin + 1) & ~1);
        // the compact form only when every channel's two replicas are exact in it;
        // otherwise the float layout and its fit check
        k->code_f16[ch] = f16_exact(code, code_samples);
        bool pack = k->pack_wanted;
        for (uint32_t i = 0; i < k->conf.max_channels; ++i) pack = pack && k->code_f16[i] && k->data_f16[i];
        const int dp = k->conf.track_pilot && !pack ? cp : 0;
        GSDR_REQUIRE(lds_for(cp, dp) <= kCuLds - kStaticLdsMargin, GSDR_E_UNSUPPORTED,
            "gsdr_trk_start: replica of %d samples does not fit the LDS next to the input window", code_samples);
        k->code_pad = cp;
        k->data_pad = dp;
        k->pack = pack;
    }
    k->lds_bytes = lds_for(k->code_pad, k->data_pad);
    GSDR_HIP(hipMemcpyAsync(k->code_bufs[ch], code, (size_t)code_samples * sizeof(float), hipMemcpyHostToDevice,
        k->stream));
    GSDR_HIP(hipMemcpyAsync(k->d_consts + ch, &c, sizeof(TrkConst), hipMemcpyHostToDevice, k->stream));
    GSDR_HIP(hipMemcpyAsync(k->d_chans + ch, &tc, sizeof(TrkChan), hipMemcpyHostToDevice, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    k->started = true;
    return GSDR_OK;
}

void gsdr_trk_kf_conf_default(gsdr_trk_kf_conf* c)  // Kf_Conf::Kf_Conf (kf_conf.cc)
{
    if (!c) return;
    c->code_disc_sd_chips = 0.2;
    c->carrier_disc_sd_rads = 0.3;
    c->code_phase_sd_chips = 0.15;
    c->carrier_phase_sd_rad = 0.25;
    c->carrier_freq_sd_hz = 0.6;
    c->carrier_freq_rate_sd_hz_s = 0.01;
    c->init_code_phase_sd_chips = 0.5;
    c->init_carrier_phase_sd_rad = 0.7;
    c->init_carrier_freq_sd_hz = 5.0;
    c->init_carrier_freq_rate_sd_hz_s = 1.0;
}

int gsdr_trk_set_kf(gsdr_trk* k, const gsdr_trk_kf_conf* conf)
{
    GSDR_REQUIRE(k && conf, GSDR_E_ARG, "gsdr_trk_set_kf: null argument");
    const double v[10] = {conf->code_disc_sd_chips, conf->carrier_disc_sd_rads, conf->code_phase_sd_chips,
        conf->carrier_phase_sd_rad, conf->carrier_freq_sd_hz, conf->carrier_freq_rate_sd_hz_s, conf->init_code_phase_sd_chips,
        conf->init_carrier_phase_sd_rad, conf->init_carrier_freq_sd_hz, conf->init_carrier_freq_rate_sd_hz_s};
    for (int i = 0; i < 10; ++i)
        GSDR_REQUIRE(std::isfinite(v[i]) && v[i] >= 0.0, GSDR_E_ARG, "gsdr_trk_set_kf: value %d (%g) is negative or not finite", i,
            v[i]);
    std::lock_guard<std::mutex> lk(k->mu);
    GSDR_REQUIRE(!k->conf.high_dyn, GSDR_E_UNSUPPORTED, "gsdr_trk_set_kf: the Kalman loop has no high-dynamics branch");
    GSDR_REQUIRE(!k->started, GSDR_E_STATE, "gsdr_trk_set_kf: a channel has been started");
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipFuncSetAttribute((const void*)trk_kernel_of(k->conf.item_type, false, true),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - kStaticLdsMargin)));
    // and the compact-replica instance this handle can launch beside it (gsdr_trk_create)
    if (k->pack_wanted)
        GSDR_HIP(hipFuncSetAttribute((const void*)trk_kernel_of(k->conf.item_type, true, true),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - kStaticLdsMargin)));
    k->kf_conf = *conf;
    k->kf = true;
    return GSDR_OK;
}

int gsdr_trk_get_kf_state(gsdr_trk* k, int ch, double x[4], double P[16])
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_get_kf_state: null handle");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_get_kf_state: channel %d", ch);
    std::lock_guard<std::mutex> lk(k->mu);
    GSDR_REQUIRE(k->kf, GSDR_E_STATE, "gsdr_trk_get_kf_state: the handle is not in Kalman mode (gsdr_trk_set_kf)");
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipStreamWaitEvent(k->stream, k->last_launch, 0));
    GSDR_HIP(hipMemcpyAsync(&k->h_chans[ch], k->d_chans + ch, sizeof(TrkChan), hipMemcpyDeviceToHost, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    const TrkKf& f = k->h_chans[ch].kf;
    if (x) std::memcpy(x, f.x, sizeof(f.x));
    if (P) std::memcpy(P, f.P, sizeof(f.P));
    return GSDR_OK;
}

int gsdr_trk_set_data_code(gsdr_trk* k, int ch, const float* data_code, int code_samples)
{
    GSDR_REQUIRE(k && data_code, GSDR_E_ARG, "gsdr_trk_set_data_code: null argument");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_set_data_code: channel %d", ch);
    GSDR_REQUIRE(k->conf.track_pilot, GSDR_E_STATE, "gsdr_trk_set_data_code: the handle does not track a pilot");
    GSDR_REQUIRE(code_samples >= 1 && code_samples <= kMaxCodeFloats, GSDR_E_UNSUPPORTED,
        "gsdr_trk_set_data_code: replica of %d samples outside [1,%d]", code_samples, kMaxCodeFloats);
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipMemcpyAsync(k->data_code_bufs[ch], data_code, (size_t)code_samples * sizeof(float),
        hipMemcpyHostToDevice, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    k->data_code_len[ch] = code_samples;
    k->data_f16[ch] = f16_exact(data_code, code_samples);
    return GSDR_OK;
}

int gsdr_trk_set_secondary_code(gsdr_trk* k, int ch, const char* bits, int len)
{
    GSDR_REQUIRE(k && bits, GSDR_E_ARG, "gsdr_trk_set_secondary_code: null argument");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_set_secondary_code: channel %d", ch);
    GSDR_REQUIRE(k->conf.signal == GSDR_SIGNAL_GAL_5X && k->conf.track_pilot, GSDR_E_STATE,
        "gsdr_trk_set_secondary_code: only a Galileo E5a pilot handle takes a per-channel secondary code");
    GSDR_REQUIRE(len >= 1 && len <= kPreambleLen, GSDR_E_ARG, "gsdr_trk_set_secondary_code: length %d outside [1,%d]", len,
        kPreambleLen);
    for (int i = 0; i < len; ++i)
        GSDR_REQUIRE(bits[i] == '0' || bits[i] == '1', GSDR_E_ARG, "gsdr_trk_set_secondary_code: character %d is not 0 / 1", i);
    std::lock_guard<std::mutex> lk(k->mu);
    k->sec_codes[ch].assign(bits, (size_t)len);
    return GSDR_OK;
}

int gsdr_trk_stop(gsdr_trk* k, int ch)
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_stop: null handle");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_stop: channel %d", ch);
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    const int32_t zero = 0;
    GSDR_HIP(hipStreamWaitEvent(k->stream, k->last_launch, 0));
    GSDR_HIP(hipMemcpyAsync(reinterpret_cast<char*>(k->d_chans + ch) + offsetof(TrkChan, h) + offsetof(TrkHot, state),
        &zero, sizeof(zero),
        hipMemcpyHostToDevice, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    return GSDR_OK;
}

// msg_handler_telemetry_to_trk (dll_pll_veml_tracking.cc:614-637): a telemetry fault
// sets d_carrier_lock_fail_counter = 200000, so the next lock check that evaluates the
// counters (states 2 / 4 with a full CN0 buffer, :986-1024) reports the loss of lock.
// Written into the channel's device state between launches, like gsdr_trk_stop.
int gsdr_trk_force_loss_of_lock(gsdr_trk* k, int ch)
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_force_loss_of_lock: null handle");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_force_loss_of_lock: channel %d", ch);
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    const int32_t forced = 200000;
    GSDR_HIP(hipStreamWaitEvent(k->stream, k->last_launch, 0));
    GSDR_HIP(hipMemcpyAsync(reinterpret_cast<char*>(k->d_chans + ch) + offsetof(TrkChan, h) +
                                offsetof(TrkHot, carrier_lock_fail_counter),
        &forced, sizeof(forced), hipMemcpyHostToDevice, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    return GSDR_OK;
}

int gsdr_trk_run_device(gsdr_trk* k, const void* iq_dev, uint64_t iq_first_sample, uint64_t iq_items, uint32_t max_epochs,
    gsdr_trk_epoch* out_dev, uint32_t* n_out_dev, void* stream)
{
    GSDR_REQUIRE(k && iq_dev && out_dev && n_out_dev, GSDR_E_ARG, "gsdr_trk_run_device: null argument");
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    hipStream_t s = stream ? (hipStream_t)stream : k->stream;
    return launch(k, iq_dev, iq_first_sample, iq_items, max_epochs, out_dev, n_out_dev, s);
}

int gsdr_trk_run_stream(gsdr_trk* k, gsdr_stream* ring, uint32_t max_epochs, gsdr_trk_epoch* out_dev,
    uint32_t* n_out_dev, void* stream)
{
    GSDR_REQUIRE(k && ring && out_dev && n_out_dev, GSDR_E_ARG, "gsdr_trk_run_stream: null argument");
    int rc = gsdr::check_ring_consumer("gsdr_trk_run_stream", ring, k->conf.item_type, k->device, "tracking");
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    hipStream_t s = stream ? (hipStream_t)stream : k->stream;
    gsdr::StreamReader rd(ring);  // ring lock from window choice to reader-event record
    uint64_t first = 0, n = 0;
    rc = rd.span(&first, &n);
    if (rc != GSDR_OK) return rc;
    const void* iq = nullptr;
    rc = rd.view(first, n, &iq);
    if (rc != GSDR_OK) return rc;
    rc = rd.acquire(s);
    if (rc != GSDR_OK) return rc;
    rc = launch(k, iq, first, n, max_epochs, out_dev, n_out_dev, s);
    if (rc != GSDR_OK) return rc;
    return rd.release(s);
}

int gsdr_trk_run_stream_host(gsdr_trk* k, gsdr_stream* ring, uint32_t max_epochs, gsdr_trk_epoch* out_host,
    uint32_t* n_out_host)
{
    GSDR_REQUIRE(k && ring && out_host && n_out_host, GSDR_E_ARG, "gsdr_trk_run_stream_host: null argument");
    {
        std::lock_guard<std::mutex> lk(k->mu);
        gsdr::DeviceGuard g(k->device);
        int rc = ensure_out(k, max_epochs);
        if (rc != GSDR_OK) return rc;
    }
    int rc = gsdr_trk_run_stream(k, ring, max_epochs, k->d_out, k->d_nout, nullptr);
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipMemcpyAsync(n_out_host, k->d_nout, k->conf.max_channels * sizeof(uint32_t), hipMemcpyDeviceToHost,
        k->stream));
    GSDR_HIP(hipMemcpyAsync(out_host, k->d_out, (size_t)k->conf.max_channels * max_epochs * sizeof(gsdr_trk_epoch),
        hipMemcpyDeviceToHost, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    return GSDR_OK;
}

int gsdr_trk_submit_stream(gsdr_trk* k, gsdr_stream* ring, uint32_t max_epochs)
{
    GSDR_REQUIRE(k && ring, GSDR_E_ARG, "gsdr_trk_submit_stream: null argument");
    GSDR_REQUIRE(max_epochs >= 1, GSDR_E_ARG, "gsdr_trk_submit_stream: max_epochs must be >= 1");
    std::lock_guard<std::mutex> submit_lk(k->submit_mu);
    gsdr_trk::Submission* u = nullptr;
    {
        std::lock_guard<std::mutex> lk(k->mu);
        GSDR_REQUIRE(k->sub_count < gsdr_trk::kSubmissions, GSDR_E_STATE,
            "gsdr_trk_submit_stream: %d submissions in flight, collect the oldest first", gsdr_trk::kSubmissions);
        gsdr::DeviceGuard g(k->device);
        const uint32_t nch = k->conf.max_channels;
        u = &k->sub[(k->sub_head + k->sub_count) % gsdr_trk::kSubmissions];
        if (max_epochs > u->cap)
            {
                // not pending: nothing in flight writes this slot's buffer
                if (u->h_out) GSDR_HIP(hipHostFree(u->h_out));
                u->h_out = nullptr;
                u->cap = 0;
                GSDR_HIP(hipHostMalloc(reinterpret_cast<void**>(&u->h_out), (size_t)nch * max_epochs * sizeof(gsdr_trk_epoch),
                    hipHostMallocMapped));
                u->cap = max_epochs;
            }
        if (!u->h_nout)
            {
                GSDR_HIP(hipHostMalloc(reinterpret_cast<void**>(&u->h_nout), nch * sizeof(uint32_t), hipHostMallocMapped));
                GSDR_HIP(hipEventCreateWithFlags(&u->done, hipEventDisableTiming));
            }
    }
    // on the handle's stream: ordered after the submissions still in flight; the
    // kernel's records land in the pinned host buffers themselves
    int rc = gsdr_trk_run_stream(k, ring, max_epochs, u->h_out, u->h_nout, nullptr);
    if (rc != GSDR_OK) return rc;
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipEventRecord(u->done, k->stream));
    u->epochs = max_epochs;
    k->sub_count++;
    return GSDR_OK;
}

int gsdr_trk_collect(gsdr_trk* k, int wait, gsdr_trk_epoch* out_host, uint32_t* n_out_host, uint32_t* max_epochs)
{
    GSDR_REQUIRE(k && out_host && n_out_host, GSDR_E_ARG, "gsdr_trk_collect: null argument");
    std::lock_guard<std::mutex> lk(k->mu);
    GSDR_REQUIRE(k->sub_count > 0, GSDR_E_STATE, "gsdr_trk_collect: nothing submitted");
    gsdr::DeviceGuard g(k->device);
    gsdr_trk::Submission& u = k->sub[k->sub_head];
    if (!wait)
        {
            const hipError_t q = hipEventQuery(u.done);
            if (q == hipErrorNotReady) return 1;
            GSDR_HIP(q);
        }
    else
        GSDR_HIP(hipEventSynchronize(u.done));
    k->sub_head = (k->sub_head + 1) % gsdr_trk::kSubmissions;
    k->sub_count--;
    const uint32_t nch = k->conf.max_channels, me = u.epochs;
    std::memcpy(n_out_host, u.h_nout, nch * sizeof(uint32_t));
    // each channel's records only (a few of max_epochs per advance)
    for (uint32_t c = 0; c < nch; ++c)
        std::memcpy(out_host + (size_t)c * me, u.h_out + (size_t)c * me, std::min(u.h_nout[c], me) * sizeof(gsdr_trk_epoch));
    if (max_epochs) *max_epochs = me;
    return GSDR_OK;
}

int gsdr_trk_run(gsdr_trk* k, const void* iq_host, uint64_t iq_first_sample, uint64_t iq_items, uint32_t max_epochs,
    gsdr_trk_epoch* out_host, uint32_t* n_out_host)
{
    GSDR_REQUIRE(k && iq_host && out_host && n_out_host, GSDR_E_ARG, "gsdr_trk_run: null argument");
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    const size_t bytes = (size_t)iq_items * gsdr::item_bytes(k->conf.item_type);
    if (iq_items > k->iq_cap)
        {
            if (k->d_iq) GSDR_HIP(hipFree(k->d_iq));
            k->d_iq = nullptr;
            k->iq_cap = 0;
            GSDR_HIP(hipMalloc(&k->d_iq, bytes));
            k->iq_cap = iq_items;
        }
    int rc = ensure_out(k, max_epochs);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(k->d_iq, iq_host, bytes, hipMemcpyHostToDevice, k->stream));
    rc = launch(k, k->d_iq, iq_first_sample, iq_items, max_epochs, k->d_out, k->d_nout, k->stream);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipMemcpyAsync(n_out_host, k->d_nout, k->conf.max_channels * sizeof(uint32_t), hipMemcpyDeviceToHost,
        k->stream));
    GSDR_HIP(hipMemcpyAsync(out_host, k->d_out, (size_t)k->conf.max_channels * max_epochs * sizeof(gsdr_trk_epoch),
        hipMemcpyDeviceToHost, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    return GSDR_OK;
}

int gsdr_trk_get_channel(gsdr_trk* k, int ch, int32_t* state, uint64_t* next_sample, double* doppler, double* cn0)
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_get_channel: null handle");
    GSDR_REQUIRE(ch >= 0 && ch < (int)k->conf.max_channels, GSDR_E_ARG, "gsdr_trk_get_channel: channel %d", ch);
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    GSDR_HIP(hipStreamWaitEvent(k->stream, k->last_launch, 0));
    GSDR_HIP(hipMemcpyAsync(&k->h_chans[ch], k->d_chans + ch, sizeof(TrkChan), hipMemcpyDeviceToHost, k->stream));
    GSDR_HIP(hipStreamSynchronize(k->stream));
    const TrkHot& t = k->h_chans[ch].h;
    if (state) *state = t.state;
    if (next_sample) *next_sample = t.next_sample;
    if (doppler) *doppler = t.carrier_doppler_hz;
    if (cn0) *cn0 = t.cn0_db_hz;
    return GSDR_OK;
}

int gsdr_trk_save_state(gsdr_trk* k, int slot, void* stream)
{
    GSDR_REQUIRE(k && (slot == 0 || slot == 1), GSDR_E_ARG, "gsdr_trk_save_state: bad argument");
    gsdr::DeviceGuard g(k->device);
    hipStream_t s = stream ? (hipStream_t)stream : k->stream;
    GSDR_HIP(hipMemcpyAsync(k->d_snap[slot], k->d_chans, k->conf.max_channels * sizeof(TrkChan), hipMemcpyDeviceToDevice, s));
    return GSDR_OK;
}

int gsdr_trk_restore_state(gsdr_trk* k, int slot, void* stream)
{
    GSDR_REQUIRE(k && (slot == 0 || slot == 1), GSDR_E_ARG, "gsdr_trk_restore_state: bad argument");
    gsdr::DeviceGuard g(k->device);
    hipStream_t s = stream ? (hipStream_t)stream : k->stream;
    GSDR_HIP(hipMemcpyAsync(k->d_chans, k->d_snap[slot], k->conf.max_channels * sizeof(TrkChan), hipMemcpyDeviceToDevice, s));
    return GSDR_OK;
}

int gsdr_trk_set_cu_mask(gsdr_trk* k, const uint32_t* mask, int n_words)
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_set_cu_mask: null handle");
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    return gsdr::replace_stream(&k->stream, mask, n_words);
}

int gsdr_trk_set_profiling(gsdr_trk* k, int enable)
{
    GSDR_REQUIRE(k, GSDR_E_ARG, "gsdr_trk_set_profiling: null handle");
    std::lock_guard<std::mutex> lk(k->mu);
    k->profiling = enable != 0;
    return GSDR_OK;
}

int gsdr_trk_read_profile(gsdr_trk* k, double* kernel_ms, uint32_t* launches)
{
    GSDR_REQUIRE(k && kernel_ms && launches, GSDR_E_ARG, "gsdr_trk_read_profile: null argument");
    std::lock_guard<std::mutex> lk(k->mu);
    gsdr::DeviceGuard g(k->device);
    *kernel_ms = 0.0;
    *launches = 0;
    for (auto& r : k->prof_recs)
        {
            GSDR_HIP(hipEventSynchronize(r.second));
            float ms = 0.0f;
            GSDR_HIP(hipEventElapsedTime(&ms, r.first, r.second));
            *kernel_ms += ms;
            *launches += 1;
            k->prof_pool.push_back(r.first);
            k->prof_pool.push_back(r.second);
        }
    k->prof_recs.clear();
    return GSDR_OK;
}

}  // extern "C"
