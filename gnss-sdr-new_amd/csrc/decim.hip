// Acquisition resampler: a decimating low-pass FIR between two device IQ rings.
//
// The reference, with GNSS-SDR.use_acquisition_resampler set, inserts one
// gr::filter::fir_filter_ccf (taps from firdes::low_pass) per signal and RF channel
// between the signal conditioner and the acquisition blocks
// (gnss_flowgraph.cc:1012-1128), so PCPS runs near 2 Msps instead of the front-end
// rate.  Here the filter reads a source ring (any item type) and produces a
// gr_complex ring every existing consumer can read.
//
// Output item m is y[m] = sum_{j<T} t[j] * x[m*d - j] over ABSOLUTE source sample
// indices, with x = 0 before the source's first pushed sample (GNU Radio's zero
// history).  An output index times d is an input sample index
// (pcps_acquisition.cc:705 maps delays back that way).
//
// Arithmetic: one fp32 FMA chain per output component, j = 0 .. T-1 in that order,
// whatever call, tile or ring wrap the output falls in: the same input gives the
// same bytes however it was pushed.
//
// Kernel layout: a workgroup stages the converted inputs of its tile in LDS
// phase-major -- the sample at distance n from the tile's origin (a multiple of d)
// sits at [n mod d][n div d] -- so for a fixed tap the lanes of a wave, which
// produce consecutive outputs, read consecutive float2 of one row: ds_read_b64
// without bank conflicts for every d, where a linear image would be read at a
// stride of d float2 (2-way at d = 2 and 10, 8-way at d = 8).  The taps are
// wave-uniform and come through the scalar cache.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <vector>

#include "gsdr_internal.h"
#include "gsdr_stream_internal.h"

namespace
{
constexpr uint32_t kMaxDecimation = 64;
constexpr uint32_t kMaxTaps = 1024;
constexpr int kThreads = 256;
constexpr uint32_t kLdsItems = 4096;  // float2 budget of the staging image (32 KiB) when the shape allows

template <int ITEM>
__device__ __forceinline__ float2 load_item(const void* __restrict__ src, int64_t i)
{
    if constexpr (ITEM == GSDR_ITEM_GR_COMPLEX)
        return static_cast<const float2*>(src)[i];
    else if constexpr (ITEM == GSDR_ITEM_CSHORT)
        {
            const short2 v = static_cast<const short2*>(src)[i];
            return make_float2(static_cast<float>(v.x), static_cast<float>(v.y));
        }
    else
        {
            const char2 v = static_cast<const char2*>(src)[i];
            return make_float2(static_cast<float>(v.x), static_cast<float>(v.y));
        }
}

struct DecimArgs
{
    int64_t src_first;  // absolute index of src[0]; samples before it count as zero
    int64_t src_end;    // one past the last source item the pass may read
    uint64_t cap;       // output ring positions
    uint64_t window;    // mirrored positions
    int64_t m_first;    // outputs [m_first, m_end)
    int64_t m_end;
    int d;
    int ntaps;
    int tile;   // outputs per workgroup
    int hq;     // columns of history: ceil((ntaps - 1) / d)
    int pitch;  // float2 per phase row
};

// src: item src_first of the source ring (contiguous up to src_end); dst: the output ring's base
template <int ITEM>
__global__ __launch_bounds__(kThreads) void decim_fir_kernel(const DecimArgs a, const void* __restrict__ src,
    const float* __restrict__ taps, float2* __restrict__ dst)
{
    extern __shared__ float2 lds[];
    const int d = a.d;
    const int64_t mt = a.m_first + static_cast<int64_t>(blockIdx.x) * a.tile;
    const int nout = static_cast<int>(min(static_cast<int64_t>(a.tile), a.m_end - mt));
    // staging: local sample n is absolute sample org + n, org a multiple of d
    const int64_t org = (mt - a.hq) * d;
    const int nloc = (nout - 1 + a.hq) * d + 1;
    int ph = static_cast<int>(threadIdx.x) % d;
    int col = static_cast<int>(threadIdx.x) / d;
    const int dph = kThreads % d, dcol = kThreads / d;
#pragma unroll 4
    for (int n = threadIdx.x; n < nloc; n += kThreads)
        {
            // an unconditional load at a clamped (always valid) index, so the unrolled loads overlap
            const int64_t g = org + n;
            const bool in = g >= a.src_first && g < a.src_end;
            const float2 v = load_item<ITEM>(src, in ? g - a.src_first : 0);
            lds[ph * a.pitch + col] = in ? v : make_float2(0.0F, 0.0F);
            ph += dph;
            col += dcol;
            if (ph >= d)
                {
                    ph -= d;
                    ++col;
                }
        }
    __syncthreads();
    for (int o = threadIdx.x; o < nout; o += kThreads)
        {
            // x[(mt + o) * d - j] is local sample (o + hq) * d - j: row (-j) mod d, column o + hq - ceil(j / d)
            const float2* row = lds + a.hq + o;
            int p = 0;
            float re = 0.0F, im = 0.0F;
            // unrolled so that a batch of tap and LDS loads is in flight; the chain order stays j ascending
#pragma unroll 8
            for (int j = 0; j < a.ntaps; ++j)
                {
                    const float t = taps[j];
                    const float2 x = row[p * a.pitch];
                    re = __builtin_fmaf(t, x.x, re);
                    im = __builtin_fmaf(t, x.y, im);
                    const bool wrap = p == 0;
                    p = wrap ? d - 1 : p - 1;
                    row -= wrap ? 1 : 0;
                }
            const uint64_t m = static_cast<uint64_t>(mt + o);
            const uint64_t pos = m % a.cap;
            const float2 y = make_float2(re, im);
            dst[pos] = y;
            if (pos < a.window) dst[a.cap + pos] = y;
        }
}

// firdes::low_pass with the Hamming window (the reference's default), restated
int low_pass_taps(double gain, double fs, double cutoff, double tw, std::vector<float>* out)
{
    int ntaps = static_cast<int>(53.0 * fs / (22.0 * tw));
    if ((ntaps & 1) == 0) ++ntaps;
    std::vector<float> taps(static_cast<size_t>(ntaps));
    const int M = (ntaps - 1) / 2;
    const double pi = 3.14159265358979323846;
    const double w0 = 2.0 * pi * cutoff / fs;
    for (int n = -M; n <= M; ++n)
        {
            const float w = ntaps > 1 ? static_cast<float>(0.54 - 0.46 * std::cos(2.0 * pi * (n + M) / (ntaps - 1))) : 1.0F;
            if (n == 0)
                taps[static_cast<size_t>(n + M)] = static_cast<float>(w0 / pi * w);
            else
                taps[static_cast<size_t>(n + M)] = static_cast<float>(std::sin(n * w0) / (n * pi) * w);
        }
    double fmax = taps[static_cast<size_t>(M)];
    for (int n = 1; n <= M; ++n) fmax += 2.0 * taps[static_cast<size_t>(n + M)];
    const double g = gain / fmax;
    for (auto& t : taps) t = static_cast<float>(t * g);
    out->swap(taps);
    return ntaps;
}
}  // namespace

struct gsdr_decim
{
    gsdr_stream* src{nullptr};
    gsdr_stream* out{nullptr};
    int device{0};
    int item_type{GSDR_ITEM_GR_COMPLEX};
    uint32_t d{1};
    uint32_t ntaps{0};
    float* d_taps{nullptr};
    int tile{64}, hq{0}, pitch{0};
    size_t lds_bytes{0};
    bool started{false};
    uint64_t next{0};  // the next output index to produce
    std::mutex mu;
};

extern "C" {

int gsdr_firdes_low_pass(double gain, double fs, double cutoff, double transition_width, float* taps, uint32_t* ntaps)
{
    GSDR_REQUIRE(taps && ntaps, GSDR_E_ARG, "gsdr_firdes_low_pass: null argument");
    GSDR_REQUIRE(fs > 0.0 && cutoff > 0.0 && cutoff <= fs / 2 && transition_width > 0.0, GSDR_E_ARG,
        "gsdr_firdes_low_pass: need 0 < cutoff <= fs/2 and transition_width > 0");
    GSDR_REQUIRE(53.0 * fs / (22.0 * transition_width) < 1e6, GSDR_E_ARG, "gsdr_firdes_low_pass: transition width too narrow");
    std::vector<float> t;
    const int n = low_pass_taps(gain, fs, cutoff, transition_width, &t);
    GSDR_REQUIRE(static_cast<uint32_t>(n) <= *ntaps, GSDR_E_ARG, "gsdr_firdes_low_pass: %d taps exceed the buffer's %u", n,
        *ntaps);
    std::copy(t.begin(), t.end(), taps);
    *ntaps = static_cast<uint32_t>(n);
    return GSDR_OK;
}

int gsdr_acq_resampler_plan(int64_t fs_in, double opt_fs, uint32_t* decimation, uint32_t* ntaps, uint32_t* latency)
{
    GSDR_REQUIRE(decimation && ntaps && latency, GSDR_E_ARG, "gsdr_acq_resampler_plan: null argument");
    GSDR_REQUIRE(fs_in > 0 && opt_fs > 0.0, GSDR_E_ARG, "gsdr_acq_resampler_plan: rates must be positive");
    *decimation = 1;
    *ntaps = *latency = 0;
    if (static_cast<double>(fs_in) <= opt_fs) return GSDR_OK;
    // Acq_Conf::ConfigureAutomaticResampler (acq_conf.cc:97-106)
    auto d = static_cast<uint32_t>(static_cast<double>(fs_in) / opt_fs);
    while (fs_in % d > 0) --d;
    if (d <= 1) return GSDR_OK;
    // gnss_flowgraph.cc:1073-1087: low_pass(1, fs, fs_d / 2.1, fs_d / 2); :1112 the latency
    const double fs_d = static_cast<double>(fs_in / d);
    std::vector<float> t;
    const int n = low_pass_taps(1.0, static_cast<double>(fs_in), fs_d / 2.1, fs_d / 2.0, &t);
    *decimation = d;
    *ntaps = static_cast<uint32_t>(n);
    *latency = static_cast<uint32_t>((n - 1) / 2);
    return GSDR_OK;
}

int gsdr_decim_create(gsdr_stream* source, uint32_t decimation, const float* taps, uint32_t ntaps, uint64_t capacity_items,
    uint64_t max_window_items, gsdr_decim** out)
{
    GSDR_REQUIRE(out, GSDR_E_ARG, "gsdr_decim_create: null argument");
    *out = nullptr;
    GSDR_REQUIRE(source && taps, GSDR_E_ARG, "gsdr_decim_create: null argument");
    GSDR_REQUIRE(decimation >= 1 && ntaps >= 1, GSDR_E_ARG, "gsdr_decim_create: decimation and tap count must be >= 1");
    GSDR_REQUIRE(decimation <= kMaxDecimation && ntaps <= kMaxTaps, GSDR_E_UNSUPPORTED,
        "gsdr_decim_create: decimation %u / %u taps outside the supported 1..%u / 1..%u", decimation, ntaps, kMaxDecimation,
        kMaxTaps);
    // one pass reads its outputs' history and at least one stride from one window of the source
    GSDR_REQUIRE(gsdr::stream_window(source) >= static_cast<uint64_t>(ntaps) + decimation, GSDR_E_ARG,
        "gsdr_decim_create: the source ring's window (%llu items) is shorter than the %u taps plus the decimation %u",
        (unsigned long long)gsdr::stream_window(source), ntaps, decimation);
    auto* h = new (std::nothrow) gsdr_decim();
    GSDR_REQUIRE(h, GSDR_E_ALLOC, "gsdr_decim_create: out of host memory");
    h->src = source;
    h->device = gsdr::stream_device(source);
    h->item_type = gsdr::stream_item_type(source);
    h->d = decimation;
    h->ntaps = ntaps;
    h->hq = static_cast<int>((ntaps - 1 + decimation - 1) / decimation);
    // outputs per workgroup: the most (in wave multiples, up to 4 per lane) whose staging image fits the budget
    int tile = 64;
    while (tile + 64 <= 4 * kThreads && decimation * static_cast<uint32_t>(tile + 64 + h->hq + 1) <= kLdsItems) tile += 64;
    h->tile = tile;
    h->pitch = (tile + h->hq) | 1;
    h->lds_bytes = static_cast<size_t>(decimation) * h->pitch * sizeof(float2);
    int rc = gsdr_stream_create(h->device, GSDR_ITEM_GR_COMPLEX, capacity_items, max_window_items, &h->out);
    if (rc != GSDR_OK)
        {
            delete h;
            return rc;
        }
    gsdr::stream_set_device_produced(h->out);
    gsdr::DeviceGuard g(h->device);
    hipError_t e = hipMalloc(&h->d_taps, ntaps * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_taps, taps, ntaps * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        {
            gsdr::set_error("gsdr_decim_create: %s", hipGetErrorString(e));
            gsdr_decim_destroy(h);
            return GSDR_E_ALLOC;
        }
    *out = h;
    return GSDR_OK;
}

void gsdr_decim_destroy(gsdr_decim* h)
{
    if (!h) return;
    gsdr_stream_destroy(h->out);  // drains the producer stream
    gsdr::DeviceGuard g(h->device);
    if (h->d_taps) (void)hipFree(h->d_taps);
    delete h;
}

int gsdr_decim_output(gsdr_decim* h, gsdr_stream** out)
{
    GSDR_REQUIRE(h && out, GSDR_E_ARG, "gsdr_decim_output: null argument");
    *out = h->out;
    return GSDR_OK;
}

int gsdr_decim_advance(gsdr_decim* h, uint64_t* out_head)
{
    GSDR_REQUIRE(h, GSDR_E_ARG, "gsdr_decim_advance: null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    gsdr::DeviceGuard g(h->device);
    // source lock, then output lock, from the views to the reader event and the commit
    gsdr::StreamReader rd(h->src);
    gsdr::StreamWriter wr(h->out);
    if (out_head) *out_head = wr.head();
    uint64_t base = 0, oldest = 0, head = 0;
    if (!rd.bounds(&base, &oldest, &head)) return GSDR_OK;  // nothing pushed yet
    const uint64_t d = h->d, T = h->ntaps;
    if (!h->started)
        {
            h->started = true;
            h->next = (base + d - 1) / d;
        }
    const uint64_t m_end = (head + d - 1) / d;  // output m is ready once source item m*d is in
    if (m_end <= h->next) return GSDR_OK;
    // the oldest source item the backlog needs: the first output's history, zero before `base`
    const uint64_t need = h->next * d > T - 1 ? std::max(base, h->next * d - (T - 1)) : base;
    GSDR_REQUIRE(need >= oldest, GSDR_E_STATE,
        "gsdr_decim_advance: the source ring no longer holds item %llu (oldest %llu): pushed more than its capacity past "
        "the decimator's cursor (output %llu)", (unsigned long long)need, (unsigned long long)oldest,
        (unsigned long long)h->next);
    const uint64_t src_window = gsdr::stream_window(h->src);
    const uint64_t out_cap = gsdr::stream_capacity(h->out);
    const hipStream_t st = wr.stream();
    int rc = rd.acquire(st);
    if (rc != GSDR_OK) return rc;
    bool launched = false;
    while (h->next < m_end)
        {
            // one pass: outputs [next, next + n) whose inputs lie in one window of the source
            const uint64_t lo = h->next * d > T - 1 ? std::max(base, h->next * d - (T - 1)) : base;
            const uint64_t first_in = h->next * d;  // >= lo
            const uint64_t room = src_window - (first_in - lo) - 1;  // items after first_in the window still holds
            const uint64_t n = std::min({m_end - h->next, room / d + 1, out_cap});
            const uint64_t hi = (h->next + n - 1) * d + 1;  // one past the newest item read, <= head
            const void* src = nullptr;
            rc = rd.view(lo, hi - lo, &src);
            if (rc != GSDR_OK) break;
            void* ring = nullptr;
            uint64_t cap = 0, window = 0;
            rc = wr.reserve(h->next, n, &ring, &cap, &window);
            if (rc != GSDR_OK) break;
            DecimArgs a{};
            a.src_first = static_cast<int64_t>(lo);
            a.src_end = static_cast<int64_t>(hi);
            auto* dst = static_cast<float2*>(ring);
            a.cap = cap;
            a.window = window;
            a.m_first = static_cast<int64_t>(h->next);
            a.m_end = static_cast<int64_t>(h->next + n);
            a.d = static_cast<int>(d);
            a.ntaps = static_cast<int>(T);
            a.tile = h->tile;
            a.hq = h->hq;
            a.pitch = h->pitch;
            const dim3 grid(static_cast<unsigned>((n + h->tile - 1) / h->tile));
            if (h->item_type == GSDR_ITEM_GR_COMPLEX)
                decim_fir_kernel<GSDR_ITEM_GR_COMPLEX><<<grid, kThreads, h->lds_bytes, st>>>(a, src, h->d_taps, dst);
            else if (h->item_type == GSDR_ITEM_CSHORT)
                decim_fir_kernel<GSDR_ITEM_CSHORT><<<grid, kThreads, h->lds_bytes, st>>>(a, src, h->d_taps, dst);
            else
                decim_fir_kernel<GSDR_ITEM_IBYTE><<<grid, kThreads, h->lds_bytes, st>>>(a, src, h->d_taps, dst);
            const hipError_t e = hipGetLastError();
            launched = true;
            if (e != hipSuccess)
                {
                    gsdr::set_error("gsdr_decim_advance: launch failed: %s", hipGetErrorString(e));
                    rc = GSDR_E_DEVICE;
                    break;
                }
            rc = wr.commit();
            if (rc != GSDR_OK) break;
            h->next += n;
        }
    // the source's reader event: a push overwriting the oldest item viewed waits for the passes
    if (launched)
        {
            const int rr = rd.release(st);
            if (rc == GSDR_OK) rc = rr;
        }
    if (out_head) *out_head = wr.head();
    return rc;
}

}  // extern "C"
