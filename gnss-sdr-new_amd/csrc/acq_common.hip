// What the acquisition translation units share and only one may define: the
// kernels that are no templates with their launch functions, the runtime switches,
// and the host helpers of the handle (view, kernel parameters, wipe-off rows,
// thresholds).
#include <cmath>
#include <cstdlib>
#include <string>

#include "acq_handle.h"

namespace
{

// ---------------------------------------------------------------- K_wipe
// One workgroup per Doppler bin; the carrier model (GSDR_WIPE_*, gsdr.h):
//   EXACT   exp(-j 2 pi f n / fs) with the phase f n / fs reduced mod 1 in fp64 and
//           cos / sin in fp64, rounded once to fp32 (the default);
//   GENERIC the generic sincos protokernel (KERN/s32f_sincos_32fc.h:390-403): lane 0
//           replays the fp32 phase accumulation sequentially, the workgroup then
//           evaluates cosf / sinf in parallel;
//   AVX2    the a_avx2 protokernel (:448-627) the reference dispatches on AVX2 x86-64:
//           lanes 0..7 replay the eight fp32 accumulators (start phase + k inc, step
//           8 inc), the workgroup evaluates the Cephes polynomials in the kernel's fp32
//           operation order (no contraction), the N % 8 tail with cosf / sinf.
__device__ __forceinline__ float2 cephes_sincos_avx2(float x0)
{
    const float FOPI = 1.27323954473516f;
    const float DP1 = -0.78515625f, DP2 = -2.4187564849853515625e-4f, DP3 = -3.77489497744594108e-8f;
    const float C0 = 2.443315711809948E-005f, C1 = -1.388731625493765E-003f, C2 = 4.166664568298827E-002f;
    const float S0 = -1.9515295891E-4f, S1 = 8.3321608736E-3f, S2 = -1.6666654611E-1f;
    const uint32_t bits = __float_as_uint(x0);
    bool sign_sin = (bits >> 31) != 0;
    float x = __uint_as_float(bits & 0x7fffffffu);
    float y = __fmul_rn(x, FOPI);
    int32_t j = (int32_t)y;  // cvttps: truncation
    j = (j + 1) & ~1;
    y = (float)j;
    const bool swap = (j & 4) != 0;
    const bool poly = (j & 2) == 0;
    x = __fadd_rn(x, __fmul_rn(y, DP1));
    x = __fadd_rn(x, __fmul_rn(y, DP2));
    x = __fadd_rn(x, __fmul_rn(y, DP3));
    const bool sign_cos = ((~(j - 2)) & 4) != 0;
    sign_sin = sign_sin != swap;
    const float z = __fmul_rn(x, x);
    float yc = __fmul_rn(C0, z);
    yc = __fadd_rn(yc, C1);
    yc = __fmul_rn(yc, z);
    yc = __fadd_rn(yc, C2);
    yc = __fmul_rn(yc, z);
    yc = __fmul_rn(yc, z);
    yc = __fsub_rn(yc, __fmul_rn(z, 0.5f));
    yc = __fadd_rn(yc, 1.0f);
    float ys = __fmul_rn(S0, z);
    ys = __fadd_rn(ys, S1);
    ys = __fmul_rn(ys, z);
    ys = __fadd_rn(ys, S2);
    ys = __fmul_rn(ys, z);
    ys = __fmul_rn(ys, x);
    ys = __fadd_rn(ys, x);
    const float sv = poly ? ys : yc, cv = poly ? yc : ys;
    return make_float2(sign_cos ? -cv : cv, sign_sin ? -sv : sv);
}

__global__ void __launch_bounds__(256) acq_wipeoff_kernel(float2* __restrict__ wipe, uint32_t N, float fs,
    int32_t doppler_max, int32_t doppler_center, int32_t doppler_step, int32_t doppler_bias,
    const float* __restrict__ freqs, int mode)
{
    const uint32_t d = blockIdx.x;
    float2* row = wipe + (size_t)d * N;
    // freqs: the step-two grid (update_grid_doppler_wipeoffs_step2, :307-314)
    const int32_t doppler = -doppler_max + doppler_center + doppler_step * (int32_t)d;
    const float freq = freqs ? freqs[d] : (float)(doppler_bias + doppler);
    if (mode == GSDR_WIPE_EXACT)
        {
            for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
                {
                    const double t = (double)freq * (double)i / (double)fs;
                    double s, c;
                    sincos(-6.283185307179586 * (t - floor(t)), &s, &c);
                    row[i] = make_float2((float)c, (float)s);
                }
            return;
        }
    const float phase_step = __fdiv_rn(__fmul_rn(6.283185307179586f, freq), fs);
    const float inc = -phase_step;
    if (mode == GSDR_WIPE_AVX2)
        {
            const uint32_t iters = N / 8;
            if (threadIdx.x < 8)
                {
                    const uint32_t k = threadIdx.x;
                    float ph = k == 0 ? 0.0f : __fmul_rn((float)k, inc);
                    const float inc8 = __fmul_rn(8.0f, inc);
                    for (uint32_t it = 0; it < iters; ++it)
                        {
                            row[8 * it + k].x = ph;
                            ph = __fadd_rn(ph, inc8);
                        }
                }
            else if (threadIdx.x == 8)
                {
                    float ph = __fmul_rn(inc, (float)(iters * 8));
                    for (uint32_t i = iters * 8; i < N; ++i)
                        {
                            row[i].x = ph;
                            ph = __fadd_rn(ph, inc);
                        }
                }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
                {
                    if (i < iters * 8)
                        row[i] = cephes_sincos_avx2(row[i].x);
                    else
                        {
                            float s, c;
                            sincosf(row[i].x, &s, &c);
                            row[i] = make_float2(c, s);
                        }
                }
            return;
        }
    if (threadIdx.x == 0)
        {
            float ph = 0.0f;
            for (uint32_t i = 0; i < N; ++i)
                {
                    row[i].x = ph;
                    ph = __fadd_rn(ph, inc);
                }
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
        {
            float s, c;
            sincosf(row[i].x, &s, &c);
            row[i] = make_float2(c, s);
        }
}

// One wave per (attempt b, PRN p): the statistic after every dwell k (the grid
// maximum of the accumulated grid, strict '>' scan order; CFAR input power of row
// (d*+D/2)%D divided by the dwell counter k+1, pcps_acquisition.cc:533), written to
// resk[(b*P + p)*K + k]; with CFAR also the decision (first positive dwell, else
// the last, :781-869) into res[b*P + p] with num_dwells.
__global__ void __launch_bounds__(64) acq_reduce_dwell_kernel(const RowStat* __restrict__ stats,
    gsdr_acq_result* __restrict__ resk, gsdr_acq_result* __restrict__ res, const uint32_t* __restrict__ prn_ids,
    AcqParams ap, uint64_t stamp0, uint64_t block_stride)
{
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t K = ap.dwells;
    bool done = false;
    for (uint32_t k = 0; k < K && !done; ++k)
        {
            const RowStat* s = stats + ((size_t)bp * K + k) * ap.D;
            float m = -1.0f;
            uint32_t dsel = 0xffffffffu, tsel = 0;
            for (uint32_t d = threadIdx.x; d < ap.D; d += 64)
                {
                    RowStat r = s[d];
                    if (r.max > m)
                        {
                            m = r.max;
                            dsel = d;
                            tsel = r.idx;
                        }
                }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                {
                    float om = __shfl_xor(m, off);
                    uint32_t od = __shfl_xor(dsel, off);
                    uint32_t ot = __shfl_xor(tsel, off);
                    if (stat_better(om, od, m, dsel))
                        {
                            m = om;
                            dsel = od;
                            tsel = ot;
                        }
                }
            gsdr_acq_result r;
            r.prn = prn_ids[p];
            r.doppler_index = dsel;
            r.code_phase = tsel;
            r.doppler_hz = doppler_of(ap, dsel);
            r.peak = m;
            r.second_peak = 0.0f;
            r.input_power = 0.0f;
            r.test_statistic = 0.0f;
            r.acq_delay_samples = (double)fmodf((float)tsel, ap.samples_per_code);
            r.samplestamp = stamp0 + (uint64_t)(b * K + k) * block_stride;
            r.positive = 0;
            r.num_dwells = (int32_t)(k + 1);
            if (ap.cfar)
                {
                    const uint32_t opp = (dsel + ap.D / 2) % ap.D;
                    const float acc = s[opp].sum;
                    const float ip = ap.step_two ? ap.ip2
                                                 : (float)((double)(acc / (float)(int32_t)ap.eff) / 2.0 / (double)(k + 1));
                    r.input_power = ip;
                    r.test_statistic = m / ip;
                    r.positive = r.test_statistic > ap.threshold ? 1 : 0;
                    done = r.positive || k + 1 == K;
                    if (done && threadIdx.x == 0) res[bp] = r;
                }
            if (threadIdx.x == 0) resk[(size_t)bp * K + k] = r;
        }
}

// Peak-ratio decision over the dwells: the first positive dwell, else the last.
__global__ void acq_decide_kernel(const gsdr_acq_result* __restrict__ resk, gsdr_acq_result* __restrict__ res,
    uint32_t K, uint32_t n)
{
    const uint32_t bp = blockIdx.x * blockDim.x + threadIdx.x;
    if (bp >= n) return;
    uint32_t k = 0;
    while (k + 1 < K && !resk[(size_t)bp * K + k].positive) ++k;
    res[bp] = resk[(size_t)bp * K + k];
}

// The lane-order copy of code spectra (lane_order_slot, or pfa_lane_order_slot for a
// variant whose correlate runs the prime-factor plan): element i of a row to slot s(i) of
// the same row of dst.  One workgroup per row; the values are copied, not recomputed.
__global__ void __launch_bounds__(256) acq_code_lane_order_kernel(const float2* __restrict__ src,
    float2* __restrict__ dst, uint32_t N, int nb1, int r1, int pfa)
{
    const float2* in = src + (size_t)blockIdx.x * N;
    float2* out = dst + (size_t)blockIdx.x * N;
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x)
        out[pfa ? pfa_lane_order_slot((int)i) : lane_order_slot((int)i, nb1, r1)] = in[i];
}

// first_vs_second_peak_statistic (:546-612) on the accumulated grid: row d* with
// the +-samples_per_chip window zeroed (wrap at d_fft_size, :580-590), first
// maximum of the rest.  One workgroup per PRN.
__global__ void __launch_bounds__(256) acq_grid_second_peak_kernel(const float* __restrict__ grid,
    gsdr_acq_result* __restrict__ res, AcqParams ap)
{
    __shared__ RowStat scratch[4];
    const uint32_t p = blockIdx.x;
    const uint32_t d = res[p].doppler_index;
    const int32_t ti = (int32_t)res[p].code_phase;
    const int32_t E = (int32_t)ap.N;
    int32_t e1 = ti - (int32_t)ap.samples_per_chip;
    int32_t e2 = ti + (int32_t)ap.samples_per_chip;
    if (e1 < 0)
        e1 = E + e1;
    else if (e2 >= E)
        e2 = e2 - E;
    const float* row = grid + ((size_t)p * ap.D + d) * ap.eff;
    float best = 0.0f, sum = 0.0f;
    uint32_t bidx = 0;
    for (uint32_t j = threadIdx.x; j < ap.eff; j += 256)
        {
            const int32_t jj = (int32_t)j;
            const bool excluded = (e1 < e2) ? (jj >= e1 && jj < e2) : (jj >= e1 || jj < e2);
            const float m = excluded ? 0.0f : row[j];
            if (stat_better(m, j, best, bidx))
                {
                    best = m;
                    bidx = j;
                }
        }
    block_reduce_stat<256>(best, bidx, sum, scratch);
    if (threadIdx.x == 0)
        {
            gsdr_acq_result r = res[p];
            r.second_peak = best;
            r.test_statistic = r.peak / best;
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
            res[p] = r;
        }
}

// ---------------------------------------------------------------- K_reduce
// One wave per (b, p).  Rows are scanned in increasing d by each lane and merged
// with the (max desc, d asc) order, reproducing the reference's strict '>' scan.
__global__ void __launch_bounds__(64) acq_reduce_kernel(const RowStat* __restrict__ stats,
    gsdr_acq_result* __restrict__ res, const uint32_t* __restrict__ prn_ids, AcqParams ap, uint64_t stamp0,
    uint64_t block_stride)
{
    const uint32_t bp = blockIdx.x;  // b*P + p
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const RowStat* s = stats + (size_t)bp * ap.D;
    float m = -1.0f;
    uint32_t dsel = 0xffffffffu, tsel = 0;
    for (uint32_t d = threadIdx.x; d < ap.D; d += 64)
        {
            RowStat r = s[d];
            if (r.max > m)
                {
                    m = r.max;
                    dsel = d;
                    tsel = r.idx;
                }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            float om = __shfl_xor(m, off);
            uint32_t od = __shfl_xor(dsel, off);
            uint32_t ot = __shfl_xor(tsel, off);
            if (stat_better(om, od, m, dsel))
                {
                    m = om;
                    dsel = od;
                    tsel = ot;
                }
        }
    if (threadIdx.x != 0) return;
    gsdr_acq_result r;
    r.prn = prn_ids[p];
    r.doppler_index = dsel;
    r.code_phase = tsel;
    r.doppler_hz = doppler_of(ap, dsel);
    r.peak = m;
    r.second_peak = 0.0f;
    r.input_power = 0.0f;
    r.test_statistic = 0.0f;
    r.acq_delay_samples = (double)fmodf((float)tsel, ap.samples_per_code);
    r.samplestamp = stamp0 + (uint64_t)b * block_stride;
    r.positive = 0;
    r.num_dwells = (int32_t)ap.counter;
    if (ap.cfar)
        {
            const uint32_t opp = (dsel + ap.D / 2) % ap.D;
            const float acc = s[opp].sum;
            // float(accumulate) / int32 in float, then / 2.0 / counter in double (pcps_acquisition.cc:533)
            const float ip =
                ap.step_two ? ap.ip2 : (float)((double)(acc / (float)(int32_t)ap.eff) / 2.0 / (double)ap.counter);
            r.input_power = ip;
            r.test_statistic = m / ip;
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
        }
    res[bp] = r;
}

int env_int(const char* name, int dflt)
{
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

}  // namespace

namespace gsdr_acq_impl
{

#ifndef GSDR_ACQ_PPW_DEFAULT
#define GSDR_ACQ_PPW_DEFAULT 1
#endif
#ifndef GSDR_ACQ_QPW_DEFAULT
#define GSDR_ACQ_QPW_DEFAULT 2
#endif

// The runtime switches, read by gsdr_acq_create into the handle (so a process may
// hold handles created under different settings):
//   GSDR_ACQ_WIPE=exact|generic|avx2  the initial carrier model (gsdr_acq_set_wipeoff
//       changes it later); default exact
//   GSDR_ACQ_XSHIFT=0  one forward spectrum per Doppler row, no reuse (grid_xmap)
//   GSDR_ACQ_FOUR_GENERIC=1  the runtime four-step (variants 20 / 22) at the sizes of
//       the packed four-step (24-27): a second parity path
//   GSDR_ACQ_SPLIT=0  the packed four-step everywhere instead of the split correlate
//       (the A/B reference and a second parity path)
//   GSDR_ACQ_SPLIT_ARG=0  the split path's selected rows recomputed on the handle's
//       FFT plan (acq_argmax_four_kernel) instead of on the split plan itself
//   GSDR_ACQ_QPW  100000 = 4 x 25000: two sub-transforms per 1024-lane workgroup
//       sharing their products (2, the default: half the workgroups, each product
//       formed once for two sub-transforms -- C5 Galileo 133.6 -> 168.0 Msps,
//       profiles/r06f) or one per 512-lane workgroup (1)
//   GSDR_ACQ_PPW  25000: two PRNs per 1024-lane workgroup sharing the X row's copies
//       (2; a launch with an odd active PRN count runs one per workgroup on the same
//       plan) or one PRN per 512-lane workgroup (1, the default)
//   GSDR_ACQ_CORR_VARIANT  a packed correlate variant (PkVariants, acq_pk.hip) other
//       than default_pk_variant's, for tests
//   GSDR_ACQ_IQCAF_ROWS_HBM=1  the IQ-CAF grid kernel's rows in device memory at every size
//       (acq_iqcaf.hip), for comparing the two forms at one size
AcqEnv read_acq_env()
{
    AcqEnv e;
    if (const char* w = std::getenv("GSDR_ACQ_WIPE"))
        {
            const std::string m(w);
            e.wipe_mode = m == "generic" ? GSDR_WIPE_GENERIC : (m == "avx2" ? GSDR_WIPE_AVX2 : GSDR_WIPE_EXACT);
        }
    e.xshift = env_int("GSDR_ACQ_XSHIFT", 1) != 0;
    e.four_generic = env_int("GSDR_ACQ_FOUR_GENERIC", 0) != 0;
    e.split = env_int("GSDR_ACQ_SPLIT", 1) != 0;
    e.split_arg = env_int("GSDR_ACQ_SPLIT_ARG", 1) != 0;
    e.qpw = env_int("GSDR_ACQ_QPW", GSDR_ACQ_QPW_DEFAULT);
    e.ppw = env_int("GSDR_ACQ_PPW", GSDR_ACQ_PPW_DEFAULT);
    e.corr_variant = env_int("GSDR_ACQ_CORR_VARIANT", -1);
    e.iqcaf_rows_hbm = env_int("GSDR_ACQ_IQCAF_ROWS_HBM", 0) != 0;
    return e;
}

// The main grid's view: every Doppler row and active PRN of the handle.
AcqView view_of(const gsdr_acq* a)
{
    AcqView v;
    v.D = a->D;
    v.nprn = a->nprn;
    v.wipe = a->d_wipe;
    v.code_fft = a->d_code_fft;
    v.code_lane = a->d_code_lane;
    v.prn = a->d_prn;
    v.xm = a->xm;
    return v;
}

int check_block_count(const gsdr_acq* a, const char* who, uint32_t n, const char* name)
{
    GSDR_REQUIRE(n > 0 && n <= a->conf.max_blocks, GSDR_E_ARG, "%s: %s %u outside [1,%u]", who, name, n,
        a->conf.max_blocks);
    return GSDR_OK;
}

int check_single_grid_handle(const gsdr_acq* a, const char* who, const char* what)
{
    GSDR_REQUIRE(!a->conf.bit_transition_flag, GSDR_E_UNSUPPORTED, "%s: no %s with bit_transition_flag", who, what);
    GSDR_REQUIRE(a->K == 1, GSDR_E_UNSUPPORTED,
        "%s: %s: every item is a grid of its own; the handle must be created with max_dwells 1 (has %u)", who, what,
        a->K);
    GSDR_REQUIRE(a->consumed == a->N, GSDR_E_UNSUPPORTED,
        "%s: %s: blocks must be fft_size items (consumed_samples %u, fft_size %u)", who, what, a->consumed, a->N);
    return GSDR_OK;
}

int read_back(gsdr_acq* a, void* dst_host, const void* src_dev, size_t bytes)
{
    GSDR_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, a->stream));
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

int row_maxima_to_host(gsdr_acq* a, uint32_t P, uint32_t D, float divisor, float* out)
{
    std::vector<RowStat> st((size_t)P * D);
    const int rc = read_back(a, st.data(), a->d_stats, st.size() * sizeof(RowStat));
    if (rc != GSDR_OK) return rc;
    for (uint32_t d = 0; d < D; ++d)
        for (uint32_t p = 0; p < P; ++p) out[(size_t)d * P + p] = st[(size_t)p * D + d].max / divisor;
    return GSDR_OK;
}

AcqParams params_of(const gsdr_acq* a, const AcqView& v)
{
    AcqParams ap{};
    ap.xm = v.xm;
    ap.N = a->N;
    ap.consumed = a->consumed;
    ap.lead_zeros = a->lead;
    ap.D = v.D;
    ap.P = v.nprn;
    ap.doppler_max = a->conf.doppler_max;
    ap.doppler_center = a->conf.doppler_center;
    ap.doppler_step = (int32_t)a->conf.doppler_step;
    ap.samples_per_code = a->conf.samples_per_code;
    ap.samples_per_chip = a->conf.samples_per_chip;
    ap.dwells = a->K;
    ap.threshold = a->threshold;
    ap.cfar = (a->conf.pfa > 0.0f || v.first_peak_only) ? 1 : 0;
    ap.eff = a->eff;
    ap.out_off = a->N - a->eff;
    ap.counter = a->K;
    if (v.step_two)
        {
            ap.step_two = 1;
            ap.center2 = v.center2;
            ap.step2 = a->st2.step;
            ap.half2 = (float)std::floor((double)a->st2.nbins / 2.0);
            ap.ip2 = v.ip2;
            ap.threshold = v.threshold2;
        }
    return ap;
}

// The forward-spectrum reuse of the main grid (XMap): with the exact carrier and
// doppler_step * N / fs = p / q in lowest terms, q <= D / 2, the q spectra of
// Doppler bins 0..q-1 (each extended by E = ((D - 1) / q) p bins) hold every row;
// else the plain layout.
static XMap grid_xmap(const gsdr_acq* a)
{
    XMap plain{a->D, 0u, a->N};
    if (a->wipe_mode != GSDR_WIPE_EXACT || !a->env.xshift) return plain;
    const int64_t fs = a->conf.fs_in;
    if (fs <= 0) return plain;
    int64_t num = (int64_t)a->conf.doppler_step * (int64_t)a->N, den = fs;
    int64_t g0 = num, g1 = den;
    while (g1)  // gcd
        {
            const int64_t t = g0 % g1;
            g0 = g1;
            g1 = t;
        }
    if (g0 <= 0) return plain;
    const int64_t p = num / g0, q = den / g0;
    if (q < 1 || 2 * q > (int64_t)a->D) return plain;
    const int64_t ext = ((int64_t)(a->D - 1) / q) * p;
    // the forward stores mirror bins i < N after bin N - 1 (out[N + i], i < ext), so
    // a Doppler span wider than fs (ext > N) would leave rows reading unwritten bins
    if (ext > (int64_t)a->N) return plain;
    // the stored spectra must fit the plain layout's allocation
    if (q * ((int64_t)a->N + ext) > (int64_t)a->D * (int64_t)a->N) return plain;
    return XMap{(uint32_t)q, (uint32_t)p, (uint32_t)(a->N + ext)};
}

int launch_wipeoff(gsdr_acq* a, float2* wipe, uint32_t rows, const float* freqs)
{
    const gsdr_acq_conf& c = a->conf;
    const bool g = !freqs;  // the main grid of the configuration, else each row from its own frequency
    hipLaunchKernelGGL(acq_wipeoff_kernel, dim3(rows), dim3(256), 0, a->stream, wipe, a->N, (float)c.fs_in,
        g ? c.doppler_max : 0, g ? c.doppler_center : 0, g ? (int32_t)c.doppler_step : 0, g ? c.doppler_bias : 0, freqs,
        a->wipe_mode);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

int launch_wipeoff_long(gsdr_acq* a, float2* wipe, uint32_t rows, uint32_t len)
{
    const gsdr_acq_conf& c = a->conf;
    hipLaunchKernelGGL(acq_wipeoff_kernel, dim3(rows), dim3(256), 0, a->stream, wipe, len, (float)c.fs_in, c.doppler_max,
        c.doppler_center, (int32_t)c.doppler_step, c.doppler_bias, (const float*)nullptr, GSDR_WIPE_EXACT);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

int rebuild_wipeoffs(gsdr_acq* a)
{
    a->xm = grid_xmap(a);
    // rows 0..q-1 suffice with the reuse (the other rows would be their shifts)
    int rc = launch_wipeoff(a, a->d_wipe, a->xm.q, nullptr);
    if (rc == GSDR_OK) rc = quicksync_rebuild_wipeoffs(a);
    if (rc != GSDR_OK) return rc;
    GSDR_HIP(hipStreamSynchronize(a->stream));
    return GSDR_OK;
}

int launch_reduce(gsdr_acq* a, const AcqParams& ap, bool dwells, uint32_t nblocks, gsdr_acq_result* res,
    const uint32_t* prn, uint64_t stamp0, uint64_t stride, hipStream_t s)
{
    if (dwells)
        hipLaunchKernelGGL(acq_reduce_dwell_kernel, dim3(nblocks * ap.P), dim3(64), 0, s, a->d_stats, a->d_resk, res,
            prn, ap, stamp0, stride);
    else
        hipLaunchKernelGGL(acq_reduce_kernel, dim3(nblocks * ap.P), dim3(64), 0, s, a->d_stats, res, prn, ap, stamp0,
            stride);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

int launch_decide(gsdr_acq* a, uint32_t n, gsdr_acq_result* res, hipStream_t s)
{
    hipLaunchKernelGGL(acq_decide_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a->d_resk, res, a->K, n);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

// Slots [first_slot, first_slot + nslots) of d_code_fft into d_code_lane.
int launch_code_lane_order(gsdr_acq* a, uint32_t first_slot, uint32_t nslots)
{
    const size_t off = (size_t)first_slot * a->N;
    hipLaunchKernelGGL(acq_code_lane_order_kernel, dim3(nslots), dim3(256), 0, a->stream, a->d_code_fft + off,
        a->d_code_lane + off, a->N, a->lane_nb1, a->lane_r1, a->lane_pfa);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

int launch_grid_second_peak(gsdr_acq* a, const AcqParams& ap, gsdr_acq_result* res, hipStream_t s)
{
    hipLaunchKernelGGL(acq_grid_second_peak_kernel, dim3(ap.P), dim3(256), 0, s, a->d_dgrid, res, ap);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

void compute_threshold(gsdr_acq* a)
{
    // calculate_threshold, pcps_acquisition.cc:894-909: effective FFT size (N/2
    // with bit transition) x bins, 2*dwells degrees of freedom (max_dwells is 1
    // with bit transition)
    const float pfa = a->conf.pfa;
    if (pfa <= 0.0f) return;
    const int num_bins = (int)(a->eff * a->D);
    const double p = std::pow(1.0 - (double)pfa, 1.0 / (double)(float)num_bins);
    a->threshold = (float)(2.0 * gsdr::gamma_p_inv_int(2 * (int)a->conf.max_dwells, p));
}

// calculate_threshold with d_step_two (:894-909): pfa2 and the narrow bin count;
// with pfa2 <= 0 the reference returns early and keeps the first-step threshold.
float step_two_threshold(const gsdr_acq* a)
{
    const float pfa = a->st2.pfa2;
    if (pfa <= 0.0f) return a->threshold;
    const int num_bins = (int)(a->eff * a->st2.nbins);
    const double p = std::pow(1.0 - (double)pfa, 1.0 / (double)(float)num_bins);
    return (float)(2.0 * gsdr::gamma_p_inv_int(2 * (int)a->conf.max_dwells, p));
}

}  // namespace gsdr_acq_impl
