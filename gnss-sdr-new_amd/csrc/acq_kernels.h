// Device side of the PCPS acquisition engine (see acq.hip for the kernel map): the
// types shared by host and kernels and the kernel templates over the FFT plan
// type.  The register four-step / split kernels are in acq_split_kernels.h; the
// kernels that are no templates are defined once, in acq_common.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fft_4step.h"
#include "fft_lds.h"
#include "fft_multi.h"
#include "fft_pk.h"
#include "fft_plan.h"
#include "gsdr_internal.h"

namespace gsdr_acq_impl
{

struct RowStat
{
    float max;
    uint32_t idx;
    float sum;
    uint32_t pad;
};

// Where the forward spectrum of (block-dwell bk, Doppler d) lives in d_X.  Doppler
// bins commensurate with the FFT bin spacing (doppler_step * N / fs = p / q in
// lowest terms, q <= D / 2) with the exact carrier (GSDR_WIPE_EXACT) make
// X_d[k] = X_{d mod q}[k + (d / q) p] an exact identity: the wipe-off of Doppler
// f + a q step is the one of f times exp(-j 2 pi a p n / N), a circular shift of
// the spectrum by a p bins.  The forward pass then computes only q spectra per
// block-dwell, each stored with its first E = ((D - 1) / q) p bins repeated after
// bin N - 1 (stride N + E), and every Doppler row is a window into one of them --
// no wrap arithmetic in the readers.  q = D, p = 0, stride = N is the plain layout
// (one spectrum per Doppler bin).
struct XMap
{
    uint32_t q;       // stored spectra per block-dwell
    uint32_t p;       // bin shift per class step
    uint32_t stride;  // complex elements per stored spectrum (N + E)
    __host__ __device__ __forceinline__ size_t off(uint32_t bk, uint32_t d) const
    {
        const uint32_t a = d / q, c = d - a * q;
        return ((size_t)bk * q + c) * stride + (size_t)a * p;
    }
};

// A code slot's Tong sequence (pcps_tong_acquisition_cc: d_dwell_count, d_tong_count, d_state),
// kept on the device between calls.  dwell_count == 0 marks a slot that has seen no item since
// its reset: its rows start from zero instead of being loaded.
struct TongSlot
{
    uint32_t dwell_count;
    uint32_t tong_count;
    uint32_t state;  // GSDR_TONG_RUNNING, _POSITIVE, _NEGATIVE
    uint32_t pad;
};

struct AcqParams
{
    XMap xm;             // forward-spectrum layout (see XMap)
    uint32_t N;          // fft size
    uint32_t consumed;   // valid samples per block
    uint32_t lead_zeros; // zero samples placed before the code (sampled_ms != ms_per_code)
    uint32_t D;
    uint32_t P;
    int32_t doppler_max;
    int32_t doppler_center;
    int32_t doppler_step;
    float samples_per_code;
    uint32_t samples_per_chip;
    uint32_t dwells;      // max_dwells K (non-coherent dwells per acquisition attempt)
    float threshold;
    int32_t cfar;
    uint32_t eff;         // effective FFT size (N/2 with bit_transition_flag, else N)
    uint32_t out_off;     // first output index of the effective window (N - eff)
    // make_two_steps narrow grid (pcps_acquisition.cc:298-305, :533-540, :717-773)
    int32_t step_two;     // 1: Doppler from center2/step2, CFAR input power kept from the coarse step
    float center2;        // d_doppler_center_step_two
    float step2;          // Acq_Conf::doppler_step2
    float half2;          // static_cast<float>(floor(num_doppler_bins_step2 / 2.0))
    float ip2;            // d_input_power of the coarse step (not recomputed in step two, :530-540)
    uint32_t counter;     // d_num_noncoherent_integrations_counter of the statistic (CFAR divisor, :534)
};

}  // namespace gsdr_acq_impl

namespace
{

using gsdr::fft::Plan;
using gsdr_acq_impl::AcqParams;
using gsdr_acq_impl::RowStat;
using gsdr_acq_impl::XMap;

// Acq_doppler_hz of Doppler row d: first step int32 arithmetic (:537); step two
// static_cast<int32_t>(center2 + (float(d) - half2) * step2) in float (:539).
__device__ __forceinline__ int32_t doppler_of(const AcqParams& ap, uint32_t d)
{
    if (ap.step_two) return (int32_t)gsdr::add_rn(ap.center2, gsdr::mul_rn(gsdr::sub_rn((float)d, ap.half2), ap.step2));
    return -ap.doppler_max + ap.doppler_center + ap.doppler_step * (int32_t)d;
}

template <int IT>
__device__ __forceinline__ float2 load_item(const void* __restrict__ p, size_t i)
{
    if constexpr (IT == GSDR_ITEM_GR_COMPLEX)
        {
            return reinterpret_cast<const float2*>(p)[i];
        }
    else if constexpr (IT == GSDR_ITEM_CSHORT)
        {
            short2 s = reinterpret_cast<const short2*>(p)[i];
            return make_float2((float)s.x, (float)s.y);
        }
    else
        {
            // Ibyte_To_Complex: interleaved_char_to_complex, scale 1 (exact)
            char2 s = reinterpret_cast<const char2*>(p)[i];
            return make_float2((float)s.x, (float)s.y);
        }
}

__device__ __forceinline__ bool stat_better(float am, uint32_t ai, float bm, uint32_t bi)
{
    return am > bm || (am == bm && ai < bi);
}

// Block-wide (max, first argmax, sum) reduction; result valid in thread 0.
template <int NT>
__device__ __forceinline__ void block_reduce_stat(float& m, uint32_t& idx, float& sum, RowStat* scratch)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            float om = __shfl_xor(m, off);
            uint32_t oi = __shfl_xor(idx, off);
            float os = __shfl_xor(sum, off);
            if (stat_better(om, oi, m, idx))
                {
                    m = om;
                    idx = oi;
                }
            sum += os;
        }
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (NW > 1)
        {
            if (lane == 0) scratch[wave] = RowStat{m, idx, sum, 0};
            __syncthreads();
            if (threadIdx.x == 0)
                {
                    for (int w = 1; w < NW; ++w)
                        {
                            RowStat s = scratch[w];
                            if (stat_better(s.max, s.idx, m, idx))
                                {
                                    m = s.max;
                                    idx = s.idx;
                                }
                            sum += s.sum;
                        }
                }
        }
}

// ---------------------------------------------------------------- K_code
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_code_fft_kernel(const float2* __restrict__ codes,
    float2* __restrict__ code_fft, const float2* __restrict__ tw, typename PT::PlanT plan, uint32_t consumed, uint32_t lead)
{
    // set_local_code (pcps_acquisition.cc:176-209): [0 x lead, code[0 .. N - lead)];
    // lead = N - consumed, or N/2 with bit_transition_flag (then only the first N/2
    // code samples of the consumed-long row are used)
    extern __shared__ float2 lds[];
    const uint32_t p = blockIdx.x;
    const float2* c = codes + (size_t)p * consumed;
    float2* out = code_fft + (size_t)p * plan.n;
    const int valid = (int)plan.n - (int)lead;
    auto load = [&](int i) -> float2 {
        int k = i - (int)lead;
        return (k >= 0 && k < valid) ? c[k] : make_float2(0.f, 0.f);
    };
    auto store = [&](int i, float2 v) { out[i] = v; };
    PT::run(plan, lds, tw, load, store);
}

// ---------------------------------------------------------------- K_forward
template <class PT, int IT>
__global__ void __launch_bounds__(PT::NT) acq_forward_kernel(const void* __restrict__ iq, uint64_t block_stride,
    const float2* __restrict__ wipe, float2* __restrict__ X, const float2* __restrict__ tw, typename PT::PlanT plan,
    uint32_t consumed, XMap xm)
{
    extern __shared__ float2 lds[];
    // blockIdx.x = block, blockIdx.y = Doppler bin (of the xm.q stored spectra):
    // the workgroups of one wipe-off row w_d are consecutive, so each XCD's L2
    // fetches the row once per launch (with d fastest every row was re-read from
    // HBM for every block)
    const uint32_t b = blockIdx.x, d = blockIdx.y;
    const size_t base = (size_t)b * block_stride;
    const float2* w = wipe + (size_t)d * plan.n;
    float2* out = X + xm.off(b, d);
    const int ext = (int)(xm.stride - plan.n);  // bins repeated after N - 1 (XMap)
    auto load = [&](int i) -> float2 {
        if (i >= (int)consumed) return make_float2(0.f, 0.f);
        return gsdr::fft::cmul(load_item<IT>(iq, base + i), w[i]);
    };
    auto store = [&](int i, float2 v) {
        out[i] = v;
        if (i < ext) out[plan.n + i] = v;
    };
    PT::run(plan, lds, tw, load, store);
}

// plan types with a packed sub-plan (FourStepPkPlan): the two-launch forward
template <class PT, class = void>
struct requires_subplan : std::false_type
{
};
template <class PT>
struct requires_subplan<PT, std::void_t<typename PT::SubPlan>> : std::true_type
{
};

// ---------------------------------------------------------------- K_forward, two launches (split path)
// The four-step forward transform of the large sizes as two launches instead of one
// workgroup per (b, d) spectrum (320 workgroups at C4 for 256 CUs -- latency-bound):
// acq_forward4_cols_kernel runs the R-point column DFTs of every (b, d) row on
// all CUs (one lane per column, coalesced loads of the wiped-off input, the
// inter-step twiddle W_N^{n2 k1}) into a scratch image of the rows k1 (N2 points
// each, contiguous); acq_forward4_rows_kernel then runs the R * nblocks * D
// sub-transforms on the packed N2-point plan, one per workgroup, storing
// X[k1 + R k2].  The R workgroups of one (b, d) share an XCD, so its L2 merges
// their interleaved output writes.  Same arithmetic as FourStepPkPlan::run.
template <class PT, int IT>
__global__ void __launch_bounds__(256) acq_forward4_cols_kernel(const void* __restrict__ iq, uint64_t block_stride,
    const float2* __restrict__ wipe, float2* __restrict__ scratch, const float2* __restrict__ tw, uint32_t consumed,
    uint32_t D)
{
    using gsdr::pk::c2;
    constexpr int R = PT::R, N2 = PT::N2, N = PT::N;
    const uint32_t row = blockIdx.y;  // b * D + d
    const uint32_t b = row / D, d = row - (row / D) * D;
    const int n2 = (int)(blockIdx.x * 256 + threadIdx.x);
    if (n2 >= N2) return;
    const size_t base = (size_t)b * block_stride;
    const float2* w = wipe + (size_t)d * N;
    c2 v[R];
#pragma unroll
    for (int n1 = 0; n1 < R; ++n1)
        {
            const int i = n1 * N2 + n2;
            v[n1] = i < (int)consumed ? gsdr::pk::from(gsdr::fft::cmul(load_item<IT>(iq, base + i), w[i]))
                                      : c2{0.0f, 0.0f};
        }
    gsdr::pk::Dft<R>::run(v);
    const gsdr::fft::ColTwiddles<R> cw(tw, n2);
    float2* out = scratch + (size_t)row * N;
    out[n2] = gsdr::pk::to(v[0]);
#pragma unroll
    for (int k1 = 1; k1 < R; ++k1) out[(size_t)k1 * N2 + n2] = gsdr::pk::to(gsdr::pk::mul(v[k1], cw(k1)));
}

template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_forward4_rows_kernel(const float2* __restrict__ scratch,
    float2* __restrict__ X, const float2* __restrict__ tw_sub, uint32_t nrows, uint32_t xstride)
{
    using gsdr::pk::c2;
    using SP = typename PT::SubPlan;
    constexpr int R = PT::R, N2 = PT::N2, N = PT::N;
    extern __shared__ float2 lds_raw[];
    // (row, k1), the R workgroups of a row on one XCD (ids dealt round-robin)
    const uint32_t id = blockIdx.x, full = nrows >> 3;
    uint32_t row, k1;
    if (id < full * 8u * R)
        {
            const uint32_t xcd = id & 7u, slot = id >> 3;
            row = (slot / R) * 8u + xcd;
            k1 = slot - (slot / R) * R;
        }
    else
        {
            const uint32_t t = id - full * 8u * R;
            row = full * 8u + t / R;
            k1 = t - (t / R) * R;
        }
    const c2* rk = reinterpret_cast<const c2*>(scratch) + (size_t)row * N + (size_t)k1 * N2;
    // stored spectrum `row` (= b q + d of XMap, d < q) with its E = xstride - N
    // repeated leading bins
    float2* out = X + (size_t)row * xstride;
    const int ext = (int)(xstride - (uint32_t)N);
    auto ld = [&](int, int, int i) -> c2 { return rk[i]; };
    auto st = [&](int k2, c2 v, int) {
        const int k = (int)k1 + R * k2;
        out[k] = gsdr::pk::to(v);
        if (k < ext) out[N + k] = gsdr::pk::to(v);
    };
    SP::template run<false>(reinterpret_cast<c2*>(lds_raw), tw_sub, ld, st, [] {});
}

// ---------------------------------------------------------------- K_correlate
// blockIdx.x = d*P + p (consecutive workgroups share the spectrum X_{b,d}), blockIdx.y = b.
// GRID: also write the full |R|^2 row (the reference's grid dump).
template <class PT, bool GRID>
__global__ void __launch_bounds__(PT::NT) acq_correlate_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, float* __restrict__ grid,
    const float2* __restrict__ tw, typename PT::PlanT plan, uint32_t D, uint32_t P, uint32_t prn_slot_for_grid, XMap xm)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    const uint32_t N = plan.n;
    uint32_t d, p, b;
    if (GRID)
        {
            d = blockIdx.x;
            p = prn_slot_for_grid;
            b = blockIdx.y;
        }
    else
        {
            // XCD-aware mapping (cdna_hip_programming.md T1): workgroups are dealt
            // round-robin over the 8 XCDs (id % 8), so give all P workgroups of one
            // (b, d) spectrum the same id % 8 — X_{b,d} is then fetched into one
            // XCD's L2 once instead of into all eight.  Speed only, never correctness.
            const uint32_t nrows = gridDim.y * D;  // (b, d) rows
            const uint32_t id = blockIdx.y * gridDim.x + blockIdx.x;
            const uint32_t full = nrows >> 3;     // rows in the XCD-balanced part
            uint32_t row;
            if (id < full * 8u * P)
                {
                    const uint32_t xcd = id & 7u, slot = id >> 3;
                    row = (slot / P) * 8u + xcd;
                    p = slot - (slot / P) * P;
                }
            else
                {
                    const uint32_t t = id - full * 8u * P;  // the last nrows % 8 rows, linear
                    row = full * 8u + t / P;
                    p = t - (t / P) * P;
                }
            b = row / D;
            d = row - b * D;
        }
    const float2* x = X + xm.off(b, d);
    const float2* c = code_fft + (size_t)p * N;
    float best = -1.0f, sum = 0.0f;
    uint32_t bidx = 0xffffffffu;
    // conj(X . conj(C)) = conj(X) . C ; |IFFT(Y)| = |FFT(conj(Y))|
    auto load = [&](int i) -> float2 {
        float2 a = x[i], k = c[i];
        return make_float2(a.x * k.x + a.y * k.y, a.x * k.y - a.y * k.x);
    };
    auto store = [&](int i, float2 v) {
        const float m = v.x * v.x + v.y * v.y;
        if (GRID) grid[(size_t)d * N + i] = m;
        if (stat_better(m, (uint32_t)i, best, bidx))
            {
                best = m;
                bidx = (uint32_t)i;
            }
        sum += m;
    };
    PT::run(plan, lds, tw, load, store);
    if (!GRID)
        {
            block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
            if (threadIdx.x == 0) stats[((size_t)b * P + p) * D + d] = RowStat{best, bidx, sum, 0};
        }
}

// ---------------------------------------------------------------- K_correlate (packed f32)
// The sequential-PRN-group kernel on the packed-f32 FFT (fft_pk.h): one workgroup
// per (row = b*D + d, group of PG PRNs), XCD-aware; the lane's first-stage inputs
// of X_{b,d} stay in VGPRs for the whole group and the next PRN's code-spectrum
// values are fetched by the hook while the current transform runs.  The last
// stage visits each lane's outputs in increasing index order, so a strict '>'
// keeps the lane's first maximum (the reference's index_max semantics).
//
// STAT 1: row (exact max, sum) only -- an order-free reduction, 2.5 VALU per output
//         instead of 7 -- and acq_argmax_pk_kernel recomputes the one row per
//         (b, p) that the grid maximum selects to find its first maximum; the
//         reported peak is then the exact |R|^2, with the reference's first-index
//         rule (32f_index_max_32u) among exact ties.
// STAT 2: row maximum only.  The CFAR statistic needs the sum of one row per
//         (b, p), the row opposite the peak (pcps_acquisition.cc:531-533), so
//         acq_argmax_pk_kernel forms it there by Parseval instead of every row
//         summing its 4000 outputs: sum_n |R[n]|^2 = N sum_k |Y[k]|^2 for the
//         unnormalised transform of Y = conj(X) C.
//
// Where a transform's code-spectrum values come from (CS):
//   kCodeVgpr    the next PRN's values are fetched into VGPRs by the hook while the
//                current transform runs (both first-stage operand sets stay live
//                through a transform: PG = 1, or plans with registers to spare);
//   kCodeDirect  loaded by the first stage itself, X resident -- for plans whose
//                registers cannot hold both operand sets (N = 16000 on 1024 lanes);
//                the code-row latency is exposed on every transform;
//   kCodeLds     X resident (but for its last XT values, see XT in the kernel), the
//                code row staged through the FFT buffer: once the
//                last stage has read its inputs and passed its barrier the buffer
//                is dead until the next transform's first stage writes it, so each
//                wave copies its share of code row q + 1 into it there with
//                buffer_load ... lds (dwordx4, no VGPRs; row element i at byte 8 i)
//                and the copy lands under the last stage's butterflies and the row
//                maximum.  The wave waits for its own copies before the statistics
//                barrier, which so also publishes the row; the next first stage
//                reads its 25 code values from LDS (consecutive lanes, conflict
//                free) and a barrier before its writes (pre() of fft_pk.h) keeps
//                any wave from overwriting values another has yet to read: 6
//                barriers per transform instead of 5, +2 N c2 of LDS traffic.  The
//                copies move whole 1 KiB pieces per wave, so the buffer is rounded
//                up to NW KiB (pk_fft_bytes) and the statistics scratch follows it.
//                Same operands, product form and order as the other two: the row
//                maxima are bit-identical.
//   kCodeLane    kCodeLds with the copies taken from the handle's lane-order rows
//                (lane_order_slot: still linear 1 KiB pieces, the LDS image equals
//                the global layout): lane j's R1 code values lie in the slots
//                j R1 + r that its own first-stage outputs go to.  A lane overwrites
//                only what it alone has read and a wave's LDS operations execute in
//                order, so there is no pre() barrier (5 per transform) and the stage
//                takes fft_pk.h's ordinary write path.  With the outputs no longer
//                all live across a barrier every X value stays resident (XT = 0) and
//                the code values are read five at a time, a group ahead of their
//                products; the wave without a first-stage butterfly skips the reads
//                and products (SKIPW of fft_pk.h).  Operands, product form and order
//                are unchanged again.
enum CodeSrc
{
    kCodeVgpr = 0,
    kCodeDirect = 1,
    kCodeLds = 2,
    kCodeLane = 3
};

// Lane order of a row for a first stage of nb1 butterflies of radix r1: input
// r of butterfly j, element i = j + nb1 r, at slot j r1 + r -- where the stage writes
// output r of butterfly j.
constexpr int lane_order_slot(int i, int nb1, int r1) { return (i % nb1) * r1 + i / nb1; }
// the map has an inverse on [0, nb1 r1) that stays inside it: a bijection
constexpr bool lane_order_bijective(int nb1, int r1)
{
    for (int i = 0; i < nb1 * r1; ++i)
        {
            const int s = lane_order_slot(i, nb1, r1);
            if (s < 0 || s >= nb1 * r1 || (s % r1) * nb1 + s / r1 != i) return false;
        }
    return true;
}

// Lane order of a row for the prime-factor first stage (PkPfaPlan4000 of fft_pk.h): natural
// element i has the coordinates n1 = 21 i mod 32 and n2 = 43 i mod 125 = 5 m + c of
// i = (125 n1 + 32 n2) mod 4000, and is input m of lane 5 n1 + c.
constexpr int pfa_lane_order_slot(int i)
{
    const int n1 = 21 * i % 32, n2 = 43 * i % 125;
    return (5 * n1 + n2 % 5) * 25 + n2 / 5;
}
// the slot map and the plan's first_index are inverses on [0, 4000): a bijection
template <class MP>
constexpr bool pfa_lane_order_bijective()
{
    for (int i = 0; i < MP::N; ++i)
        {
            const int s = pfa_lane_order_slot(i);
            if (s < 0 || s >= MP::N || MP::first_index(s / MP::R1, s % MP::R1) != i) return false;
        }
    return true;
}
// each lane's R1 elements are one residue class mod NB1 (the 25 x 16 x 10 plan's classes, in
// an order rotated per lane)
template <class MP>
constexpr bool pfa_lane_classes()
{
    for (int j = 0; j < MP::NB1; ++j)
        for (int m = 1; m < MP::R1; ++m)
            if (MP::first_index(j, m) % MP::NB1 != MP::first_index(j, 0) % MP::NB1) return false;
    return true;
}
// the slots follow the data: middle-stage lane j = 125 e + 25 c + k25 reads, as its input m',
// the first stage's output k25 of lane 5 (2 m' + e) + c, writes only slots that it read, and
// its output k16 is the last stage's input (e, c) of butterfly (k16, k25)
template <class MP>
constexpr bool pfa_slots_chain()
{
    for (int j = 0; j < MP::NB2; ++j)
        {
            const int e = j / 125, c = j / 25 % 5, k25 = j % 25;
            for (int r = 0; r < MP::R2; ++r)
                {
                    if (MP::middle_slot(j, r) != MP::first_slot(5 * (2 * r + e) + c, k25)) return false;
                    if (MP::middle_slot(j, r) != MP::last_slot(r, k25, e, c)) return false;
                    if (MP::middle_slot(j, r) % MP::NB2 != j || MP::middle_slot(j, r) >= MP::N) return false;
                }
        }
    return true;
}
// every frequency leaves the last stage once
template <class MP>
constexpr bool pfa_outputs_bijective()
{
    bool seen[MP::N] = {};
    for (int j = 0; j < MP::NSL; ++j)
        for (int r = 0; r < MP::RL; ++r)
            {
                const int f = MP::output_index(j % 16, j / 16, r / 5, r % 5);
                if (f < 0 || f >= MP::N || seen[f]) return false;
                seen[f] = true;
            }
    return true;
}
static_assert(pfa_lane_order_bijective<gsdr::pk::PkPfaPlan4000<256>>(), "prime-factor lane order");
static_assert(pfa_lane_classes<gsdr::pk::PkPfaPlan4000<256>>(), "prime-factor first stage: residue classes mod 160");
static_assert(pfa_slots_chain<gsdr::pk::PkPfaPlan4000<256>>(), "prime-factor middle stage in place");
static_assert(pfa_outputs_bijective<gsdr::pk::PkPfaPlan4000<256>>(), "prime-factor output map");

// bytes of the FFT buffer in front of the kernel's statistics scratch
template <class MP, int CS>
constexpr size_t pk_fft_bytes()
{
    constexpr size_t piece = (size_t)(MP::NT / 64) * 1024;
    return CS == kCodeLds || CS == kCodeLane ? (MP::lds_bytes() + piece - 1) / piece * piece : MP::lds_bytes();
}

// Where the inter-stage twiddles of a three-stage plan R1 x R2 x RL come from (TW):
//   kTwGlobal  the handle's table tw, a root per butterfly (fft_pk.h TWP): a global
//              load and its wait in every transform, and the power chain w^2 .. of
//              the middle stage recomputed in every transform;
//   kTwLds     two tables in the workgroup's LDS behind the statistics scratch, built
//              once per workgroup ahead of the barrier that publishes code row 0 and
//              never written again.  The middle stage's holds the powers w^r of
//              w = tw[k RL], r = 1 .. R2-1, k < R1, formed by apply_powers' own chain
//              (the bits the registers held), r-major: lanes of equal k read one
//              address, and the stage multiplies v[r] by its entry -- no chain, R2-2
//              complex products fewer per butterfly.  The last stage's is a copy of
//              its roots tw[0 .. R1 R2); it keeps its chain.  Both are read beside the
//              stage's inputs, ahead of its barrier.
// The factors are the same in both, so are the results.  Measured on the way and not
// kept (profiles/tw99): the roots alone from LDS with both chains kept (within noise),
// and the power table read as the ds_read2_b64 pairs the compiler forms (-2 %: the
// pairs are banked mod 32, where the wrap of k at R1 = 25 makes two lanes of a
// 16-lane group collide; the conflict cycles nearly doubled).
//   kTwPfa     the prime-factor plan's (PkPfaPlan4000: no middle-stage twiddles): the 16
//              roots W_32^k and the 25 roots W_125^k, copied from tw once per workgroup into
//              the same place; the last stage forms W_125^(c k), c = 2 .. 4, by a chain.
//              Measured and not kept (profiles/pfa101): the 100 powers W_125^(c k) tabled,
//              four reads per pass instead of one and three products (-2 %).
enum TwSrc
{
    kTwGlobal = 0,
    kTwLds = 1,
    kTwPfa = 2
};

// middle-stage table: entry of w^r (1 <= r < r2) for root k of ns2; its elements
constexpr int tw_mid_index(int r, int k, int ns2) { return (r - 1) * ns2 + k; }
constexpr int tw_mid_elems(int tw, int r2, int ns2) { return tw == kTwLds ? (r2 - 1) * ns2 : 0; }
// last-stage table: a copy of tw[0 .. ns3)
constexpr int tw_last_elems(int tw, int ns3) { return tw == kTwLds ? ns3 : 0; }

// The correlate kernel's dynamic LDS: the FFT buffer, two sets of per-wave row
// statistics, the twiddle tables (middle, then last).
template <class MP, int CS>
constexpr size_t pk_tw_offset()
{
    return pk_fft_bytes<MP, CS>() + (size_t)2 * (MP::NT / 64) * sizeof(RowStat);
}
template <class MP, int TW>
constexpr size_t pk_tw_bytes()
{
    constexpr int R2 = MP::N / (MP::R1 * MP::RL);
    if (TW == kTwPfa) return (size_t)(16 + 25) * sizeof(gsdr::pk::c2);
    return (size_t)(tw_mid_elems(TW, R2, MP::R1) + tw_last_elems(TW, MP::NSL)) * sizeof(gsdr::pk::c2);
}
template <class MP, int CS, int TW>
constexpr size_t pk_corr_lds_bytes()
{
    return pk_tw_offset<MP, CS>() + pk_tw_bytes<MP, TW>();
}

// fft_pk.h twiddle source on those tables (middle stage of radix R2 after NS2 = R1)
template <int R2, int NS2>
struct TwLds
{
    const gsdr::pk::c2* mid;
    const gsdr::pk::c2* last;
    template <int R>
    struct Mid
    {
        gsdr::pk::c2 w[R - 1];
    };
    // Single ds_read_b64 in inline assembly: banked mod 64, the NS2 <= 32 entries of a
    // row never conflict and equal k broadcast.  The compiler does not count these
    // reads, so middle() waits for them itself; they return in order with the
    // compiler's own LDS reads, whose counted waits they can only lengthen.
    template <int R, int I>
    __device__ __forceinline__ static void read_powers(Mid<R>& m, unsigned a)
    {
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(m.w[I - 1]) : "v"(a), "n"(tw_mid_index(I, 0, NS2) * 8));
        if constexpr (I + 1 < R) read_powers<R, I + 1>(m, a);
    }
    template <int R, int Ns>
    __device__ __forceinline__ Mid<R> load_middle(int k) const
    {
        static_assert(R == R2 && Ns == NS2 && NS2 <= 32, "the plan's middle stage");
        Mid<R> m;
        read_powers<R, 1>(m, (unsigned)(uintptr_t)(gsdr_lvoid*)const_cast<gsdr::pk::c2*>(mid + k));
        return m;
    }
    template <int R>
    __device__ __forceinline__ void middle(gsdr::pk::c2* v, const Mid<R>& m) const
    {
        Mid<R> t = m;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int r = 1; r < R; ++r) asm volatile("" : "+v"(t.w[r - 1]));
#pragma unroll
        for (int r = 1; r < R; ++r) v[r] = gsdr::pk::mul(v[r], t.w[r - 1]);
    }
    __device__ __forceinline__ gsdr::pk::c2 last_root(int k) const { return last[k]; }
};

// PkPfaPlan4000's twiddle source on the kTwPfa tables: t32[k] = W_32^k, k < 16, then
// t125[k] = W_125^k, k < 25.  Lanes of equal k25 read one address, the 16 roots of a group
// lie in 32 consecutive dwords.
struct TwPfa
{
    const gsdr::pk::c2* t32;
    const gsdr::pk::c2* t125;
    // once per workgroup, every lane its share, from the handle's table tw[m] = W_4000^m
    __device__ __forceinline__ static void build(gsdr::pk::c2* t32, const float2* __restrict__ tw, int nt)
    {
        gsdr::pk::c2* t125 = t32 + 16;
        for (int k = (int)threadIdx.x; k < 16; k += nt) t32[k] = gsdr::pk::from(tw[125 * k]);
        for (int k = (int)threadIdx.x; k < 25; k += nt) t125[k] = gsdr::pk::from(tw[32 * k]);
    }
    __device__ __forceinline__ gsdr::pk::c2 root32(int k) const { return t32[k]; }
    __device__ __forceinline__ gsdr::pk::c2 root125(int k) const { return t125[k]; }
};

template <class MP, int PG, int WPE, int STAT, int CS, int TW = kTwGlobal>
__global__ void __launch_bounds__(MP::NT) __attribute__((amdgpu_waves_per_eu(WPE))) acq_correlate_pk_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, const float2* __restrict__ tw, uint32_t D,
    uint32_t P, uint32_t nblocks, XMap xm)
{
    static_assert(PG > 0, "PRN group");
    static_assert(CS == kCodeVgpr || CS == kCodeDirect || CS == kCodeLds || CS == kCodeLane, "code source");
    static_assert(TW == kTwGlobal || TW == kTwLds || TW == kTwPfa, "twiddle source");
    constexpr bool PFA = MP::PRIME_FACTOR;
    static_assert(PFA == (TW == kTwPfa), "the prime-factor plan and its tables go together");
    static_assert(!PFA || (CS == kCodeLane && STAT == 2), "prime-factor plan: lane-order code rows, row maximum only");
    constexpr bool PREFETCH = CS == kCodeVgpr;
    constexpr bool LANE = CS == kCodeLane;
    constexpr bool STAGED = CS == kCodeLds || LANE;
    constexpr bool TABLES = TW != kTwGlobal;
    // the tables are published by the barrier behind stage_code(0), and lie beyond
    // everything written later: the code rows' last piece ends with the padded
    // buffer, the statistics scratch follows it
    static_assert(!TABLES || (STAGED && MP::nstages == 3 && MP::TWP), "twiddle tables: a staged three-stage TWP plan");
    static_assert(!STAGED || pk_fft_bytes<MP, CS>() % ((MP::NT / 64) * 1024) == 0, "whole pieces fill the padded buffer");
    static_assert(pk_tw_offset<MP, CS>() >= pk_fft_bytes<MP, CS>() + 2 * (MP::NT / 64) * sizeof(RowStat), "tables behind the scratch");
    static_assert(!TABLES || pk_tw_offset<MP, CS>() % sizeof(gsdr::pk::c2) == 0, "table alignment");
    // four workgroups per CU: 160 KiB / 4
    static_assert(!TABLES || pk_corr_lds_bytes<MP, CS, TW>() <= 40960, "LDS of four workgroups per CU");
    static_assert(!LANE || (MP::BPT1 == 1 && (PFA || lane_order_bijective(MP::NB1, MP::R1))), "lane order of the first stage");
    // kCodeLds: the last XT of the lane's R1 X values are not resident either: all
    // R1 of them beside the last stage's two passes and the first radix's working
    // set do not fit the 128 VGPRs of four workgroups per CU (the compiler spilled
    // 10), so the first stage loads those itself, as kCodeDirect loads the code.
    // kCodeLane holds all R1 (its outputs are not all live across a barrier).
    constexpr int XT = CS == kCodeLds ? (MP::R1 + 4) / 5 : 0;
    // kCodeLane: the code values are read RA at a time, one group ahead of its products
    constexpr int RA = LANE ? 5 : 0;
    static_assert(STAT == 1 || STAT == 2, "row statistic 1 (max + sum) or 2 (max)");
    using gsdr::pk::c2;
    constexpr int NT = MP::NT;
    constexpr int NW = NT / 64;
    constexpr int R1 = MP::R1, BPT1 = MP::BPT1, NB1 = MP::NB1;
    constexpr uint32_t N = MP::N;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    RowStat* scratch = reinterpret_cast<RowStat*>(lds_raw + pk_fft_bytes<MP, CS>() / sizeof(float2));
    const uint32_t G = (P + PG - 1) / PG;
    const uint32_t nrows = nblocks * D;
    const uint32_t id = blockIdx.x;
    const uint32_t full = nrows >> 3;
    uint32_t row, g;
    if (id < full * 8u * G)
        {
            const uint32_t xcd = id & 7u, slot = id >> 3;
            row = (slot / G) * 8u + xcd;
            g = slot - (slot / G) * G;
        }
    else
        {
            const uint32_t t = id - full * 8u * G;
            row = full * 8u + t / G;
            g = t - (t / G) * G;
        }
    const uint32_t b = row / D, d = row - (row / D) * D;
    const uint32_t p0 = g * PG;
    const int np = (int)min((uint32_t)PG, P - p0);
    // the twiddle source: the tables behind the statistics scratch (built below)
    constexpr int R2 = MP::N / (MP::R1 * MP::RL);
    using Tws = std::conditional_t<PFA, TwPfa, std::conditional_t<TABLES, TwLds<R2, MP::R1>, gsdr::pk::TwGlobal>>;
    Tws tws{};
    (void)tws;
    if constexpr (PFA)
        {
            tws.t32 = lds + pk_tw_offset<MP, CS>() / sizeof(c2);
            tws.t125 = tws.t32 + 16;
        }
    else if constexpr (TABLES)
        {
            tws.mid = lds + pk_tw_offset<MP, CS>() / sizeof(c2);
            tws.last = tws.mid + tw_mid_elems(TW, R2, MP::R1);
        }
    // the X row and the code spectra through buffer descriptors built from
    // wave-uniform values: per-lane byte offset j*8 in voffset, r*NB1*8 as the
    // scalar/immediate offset -- no 64-bit address arithmetic per load
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(X) + xm.off(b, d), 0, (int)(N * sizeof(c2)), 0x00020000);
    const auto crs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(code_fft) + (size_t)p0 * N, 0, (int)((size_t)np * N * sizeof(c2)), 0x00020000);
    auto bload = [](decltype(xrs) rs, int voff, int soff) -> c2 {
        const auto u = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
        return c2{__uint_as_float(u[0]), __uint_as_float(u[1])};
    };
    // a wave with any first-stage butterfly loads for all its lanes (the idle
    // lanes' clamped, in-bounds copies keep every register defined, so no
    // zero-fill code); a wave with none skips the loads
    c2 xr[BPT1][R1], cr[BPT1][R1];
#pragma unroll
    for (int bb = 0; bb < BPT1; ++bb)
        {
            const int j = (int)threadIdx.x + bb * NT;
            const int j0 = (int)(threadIdx.x & ~63u) + bb * NT;
            if (NB1 % NT == 0 || j0 < NB1)
                {
                    const int jj = min(j, NB1 - 1);
                    if constexpr (PFA)
                        {
                            // the lane's residue class in the plan's rotated order: one wrap per
                            // load, here only
                            int i = MP::first_index(jj, 0);
#pragma unroll
                            for (int r = 0; r < R1; ++r)
                                {
                                    xr[bb][r] = bload(xrs, i * 8, 0);
                                    i += NB1;
                                    i = i >= (int)N ? i - (int)N : i;
                                }
                        }
                    else
                        {
#pragma unroll
                            for (int r = 0; r < R1 - XT; ++r)
                                {
                                    xr[bb][r] = bload(xrs, jj * 8, r * NB1 * 8);
                                    if constexpr (PREFETCH) cr[bb][r] = bload(crs, jj * 8, r * NB1 * 8);
                                }
                        }
                }
        }
    // kCodeLds: this wave's 1 KiB pieces of code row qn into the FFT buffer (lane
    // part in voffset, the row and the piece as the uniform scalar offset); the
    // last piece may run past the row's end -- into the next row, or past the
    // descriptor's (zeros) -- and lands in the buffer's padding, which no lane reads
    auto stage_code = [&](int qn) {
        constexpr int PIECE = NW * 1024;
        constexpr int PIECES = (int)(pk_fft_bytes<MP, CS>() / PIECE);
        // (uniform: the destination goes to M0)
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        char* dst = reinterpret_cast<char*>(lds_raw) + wave * 1024;
        const int voff = (int)threadIdx.x * 16;
#pragma unroll
        for (int k = 0; k < PIECES; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(crs, (gsdr_lvoid*)(dst + k * PIECE), 16, voff,
                qn * (int)(N * 8) + k * PIECE, 0, 0);
    };
    if constexpr (STAGED)
        {
            stage_code(0);
            if constexpr (PFA)
                Tws::build(lds + pk_tw_offset<MP, CS>() / sizeof(c2), tw, NT);
            else if constexpr (TABLES)
                {
                    // the twiddle tables, once per workgroup, their loads in flight beside the
                    // X row's and code row 0's: every lane copies its share of the last
                    // stage's roots, lane k < R1 runs apply_powers' chain on its middle-stage
                    // root and stores each power.  The barrier that publishes code row 0
                    // publishes them.
                    c2* tmid = lds + pk_tw_offset<MP, CS>() / sizeof(c2);
                    c2* tlast = tmid + tw_mid_elems(TW, R2, MP::R1);
#pragma unroll
                    for (int k = (int)threadIdx.x; k < MP::NSL; k += NT) tlast[k] = gsdr::pk::from(tw[k]);
                    for (int k = (int)threadIdx.x; k < MP::R1; k += NT)
                        {
                            const c2 w1 = gsdr::pk::from(tw[k * MP::RL]);
                            c2 w = w1;
#pragma unroll
                            for (int r = 1; r < R2; ++r)
                                {
                                    if (r > 1) w = gsdr::pk::mul(w, w1);
                                    tmid[tw_mid_index(r, k, MP::R1)] = w;
                                }
                        }
                }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    for (int q = 0; q < np; ++q)
        {
            {
                    float rmax = 0.0f, sum = 0.0f;
                    if constexpr (XT > 0)
                        {
                            // the X values that are not resident, issued ahead of the
                            // first stage's LDS reads (fenced: the scheduler sank the
                            // last of them behind the products, a second exposed wait)
#pragma unroll
                            for (int bb = 0; bb < BPT1; ++bb)
                                {
                                    const int jj = min((int)threadIdx.x + bb * NT, NB1 - 1);
#pragma unroll
                                    for (int r = R1 - XT; r < R1; ++r) xr[bb][r] = bload(xrs, jj * 8, r * NB1 * 8);
                                }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    c2 cb[2][RA > 0 ? RA : 1];
                    auto load = [&](int bb, int r, int i) -> c2 {
                        if constexpr (PREFETCH)
                            return gsdr::pk::conj_mul(xr[bb][r], cr[bb][r]);
                        else if constexpr (STAGED)
                            {
                                // the resident products first, while the others' X values arrive
                                if (XT > 0 && r == R1 - XT) __builtin_amdgcn_sched_barrier(0);
                                // kCodeLane: the lane's own output slots (an idle lane of a
                                // half-filled wave reads the last butterfly's, as it loads its X),
                                // group g + 1 issued before group g's products, fenced so
                                // that the scheduler keeps the reads ahead
                                if constexpr (LANE)
                                    {
                                        const c2* row = lds + min((int)threadIdx.x, NB1 - 1) * R1;
                                        if (r % RA == 0)
                                            {
                                                if (r == 0)
                                                    {
#pragma unroll
                                                        for (int k = 0; k < RA; ++k) cb[0][k] = row[k];
                                                    }
                                                const int g = r / RA + 1;
#pragma unroll
                                                for (int k = 0; k < RA; ++k)
                                                    if (g * RA + k < R1) cb[g & 1][k] = row[g * RA + k];
                                                __builtin_amdgcn_sched_barrier(0);
                                            }
                                        return gsdr::pk::conj_mul(xr[bb][r], cb[(r / RA) & 1][r % RA]);
                                    }
                                return gsdr::pk::conj_mul(xr[bb][r], lds[i]);
                            }
                        else
                            return gsdr::pk::conj_mul(xr[bb][r], bload(crs, i * 8, (int)(q * N * 8)));
                    };
                    auto hook = [&]() {
                        if (PREFETCH && q + 1 < np)
                            {
#pragma unroll
                                for (int bb = 0; bb < BPT1; ++bb)
                                    {
                                        const int j = (int)threadIdx.x + bb * NT;
                                        if (NB1 % NT == 0 || j < NB1)
                                            {
#pragma unroll
                                                for (int r = 0; r < R1; ++r)
                                                    cr[bb][r] = bload(crs, j * 8, (int)((q + 1) * N * 8) + r * NB1 * 8);
                                            }
                                    }
                            }
                    };
                    auto store = [&](int, c2 v, int) {
                        const float m = __builtin_fmaf(v.x, v.x, v.y * v.y);
                        rmax = __builtin_fmaxf(rmax, m);
                        if constexpr (STAT == 1) sum += m;
                    };
                    // two outputs at once from a plan with PAIRS, their real parts in re and their
                    // imaginary parts in im: both |z|^2 in one packed product and one packed
                    // fused multiply-add -- the roundings of store's fmaf(x, x, y * y) --, the
                    // maximum of three in one instruction
                    auto store_pair = [&](c2 re, c2 im) {
                        static_assert(!MP::PAIRS || STAT == 2, "pairs: row maximum only");
                        const c2 m = __builtin_elementwise_fma(re, re, im * im);
                        rmax = __builtin_fmaxf(__builtin_fmaxf(rmax, m.x), m.y);
                    };
                    static_assert(!MP::PAIRS || LANE, "plans with pairs: lane-order code rows");
                    if constexpr (STAGED)
                        {
                            // every wave has read its code values before any overwrites the buffer
                            auto pre = [&]() { __syncthreads(); };
                            // the buffer is dead: the next code row into it, under the butterflies
                            auto mid = [&]() {
                                if (q + 1 < np) stage_code(q + 1);
                            };
                            if constexpr (MP::PAIRS)
                                MP::template run<false, true>(lds, tw, load, gsdr::pk::PairStore<decltype(store), decltype(store_pair)>{store, store_pair},
                                    hook, gsdr::pk::NoHook{}, mid, tws);
                            else if constexpr (LANE)
                                MP::template run<false, true>(lds, tw, load, store, hook, gsdr::pk::NoHook{}, mid, tws);
                            else
                                MP::template run<false>(lds, tw, load, store, hook, pre, mid);
                        }
                    else
                        MP::template run<false>(lds, tw, load, store, hook);
                    rmax = gsdr::wave_max(rmax);
                    if constexpr (STAT == 1)
                        {
#pragma unroll
                            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
                        }
                    RowStat* sc = scratch + (q & 1) * NW;
                    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
                    if (lane == 0) sc[wave] = RowStat{rmax, 0u, sum, 0};
                    // the wave's own copies have landed; the barrier publishes the row
                    if constexpr (STAGED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (threadIdx.x == 0)
                        {
                            RowStat best = sc[0];
#pragma unroll
                            for (int w = 1; w < NW; ++w)
                                {
                                    best.max = __builtin_fmaxf(best.max, sc[w].max);
                                    best.sum += sc[w].sum;
                                }
                            stats[((size_t)b * P + p0 + q) * D + d] = best;
                        }
            }
        }
}

// After acq_reduce_kernel chose the Doppler row d* of (b, p) from the split
// kernel's row maxima: recompute row d* on the plan PT (FourStepPkPlan) -- its
// first maximum over the effective window [N - eff, N) with the reference's
// index_max rule (KERN/32f_index_max_32u.h:446-467), code_phase and
// Acq_delay_samples (pcps_acquisition.cc:709), the peak as recomputed -- and the
// CFAR power of the row opposite the peak (:531-533): by Parseval over the whole
// row, or, for the half window of bit transition, by recomputing that row too.
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_argmax_four_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ res, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap)
{
    constexpr int NT = PT::NT;
    constexpr int NW = NT / 64;
    extern __shared__ float2 lds[];
    __shared__ unsigned long long s_key[NW];
    __shared__ float s_sum[NW];
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t N = ap.N;
    const uint32_t d = res[bp].doppler_index;
    if (d >= ap.D) return;  // uniform: no maximum found (an all-NaN grid)
    const float2* c = code_fft + (size_t)p * N;
    const int off = (int)ap.out_off;
    auto row_load = [&](const float2* x) {
        return [x, c](int i) -> float2 {
            const float2 a = x[i], k = c[i];
            return make_float2(a.x * k.x + a.y * k.y, a.x * k.y - a.y * k.x);
        };
    };
    unsigned long long key = 0ull;
    auto store = [&](int i, float2 v) {
        const int j = i - off;
        if (j < 0) return;
        const float m = __builtin_fmaf(v.x, v.x, v.y * v.y);
        const unsigned long long k = ((unsigned long long)__float_as_uint(m) << 32) | (0xffffffffu - (uint32_t)j);
        key = k > key ? k : key;
    };
    PT::run(plan, lds, tw, row_load(X + ap.xm.off(b, d)), store);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        {
            const unsigned long long t = __shfl_xor(key, o);
            key = t > key ? t : key;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) key = s_key[w] > key ? s_key[w] : key;
    const uint32_t idx = 0xffffffffu - (uint32_t)(key & 0xffffffffu);
    const float peak = __uint_as_float((uint32_t)(key >> 32));
    float ip = 0.0f;
    if (ap.cfar && !ap.step_two)
        {
            const uint32_t opp = (d + ap.D / 2) % ap.D;
            const float2* xo = X + ap.xm.off(b, opp);
            float acc = 0.0f;
            if (off == 0)
                {
                    // accumulate(|R|^2) / fft_size = sum_k |Y_opp[k]|^2 (unnormalised R = FFT(conj Y))
                    for (uint32_t i = threadIdx.x; i < N; i += NT)
                        {
                            const float2 a = xo[i], k = c[i];
                            const float yr = a.x * k.x + a.y * k.y, yi = a.x * k.y - a.y * k.x;
                            acc = __builtin_fmaf(yr, yr, __builtin_fmaf(yi, yi, acc));
                        }
                }
            else
                {
                    auto sum_store = [&](int i, float2 v) {
                        if (i >= off) acc += __builtin_fmaf(v.x, v.x, v.y * v.y);
                    };
                    __syncthreads();  // LDS reuse by the second transform
                    PT::run(plan, lds, tw, row_load(xo), sum_store);
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) s_sum[wave] = acc;
            __syncthreads();
            float tot = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += s_sum[w];
            // float(accumulate) / eff, then / 2.0 / counter in double (pcps_acquisition.cc:533)
            ip = off == 0 ? (float)((double)tot / 2.0 / (double)ap.counter)
                          : (float)((double)(tot / (float)(int32_t)ap.eff) / 2.0 / (double)ap.counter);
        }
    if (threadIdx.x == 0)
        {
            gsdr_acq_result r = res[bp];
            r.code_phase = idx;
            r.acq_delay_samples = (double)fmodf((float)idx, ap.samples_per_code);
            r.peak = peak;
            if (ap.cfar)
                {
                    if (!ap.step_two) r.input_power = ip;
                    r.test_statistic = r.peak / r.input_power;
                    r.positive = r.test_statistic > ap.threshold ? 1 : 0;
                }
            res[bp] = r;
        }
}

// ---------------------------------------------------------------- K_argmax (packed f32)
// After acq_reduce_kernel chose the grid maximum's Doppler row d* of (b, p) from
// STAT-1 row maxima: recompute that row with the same packed plan and load
// functor (bit-identical values) and find its first maximum with a 64-bit key
// (|R|^2 bits, ~index) -- volk_gnsssdr_32f_index_max_32u's strict '>' scan
// (KERN/32f_index_max_32u.h:446-467) -- then write code_phase and
// Acq_delay_samples = fmod(indext, samples_per_code) (pcps_acquisition.cc:709).
// PEAK: also write the recomputed maximum as the record's peak, ahead of the statistics
// formed from it -- for a variant whose correlate runs another plan than MP (its row
// maximum is the same value rounded in another order): the record is then MP's own, bit
// for bit, whenever the same Doppler row wins.
template <class MP, int STAT, bool PEAK = false>
__global__ void __launch_bounds__(MP::NT) acq_argmax_pk_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ res, const float2* __restrict__ tw, uint32_t D,
    uint32_t P, float samples_per_code, AcqParams ap)
{
    using gsdr::pk::c2;
    constexpr int NT = MP::NT;
    constexpr int NW = NT / 64;
    constexpr uint32_t N = MP::N;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    unsigned long long* scratch = reinterpret_cast<unsigned long long*>(lds_raw + MP::lds_bytes() / sizeof(float2));
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / P, p = bp - b * P;
    const uint32_t d = res[bp].doppler_index;
    if (d >= D) return;  // uniform: no maximum found (an all-NaN grid)
    const c2* x = reinterpret_cast<const c2*>(X) + ap.xm.off(b, d);
    const c2* c = reinterpret_cast<const c2*>(code_fft) + (size_t)p * N;
    unsigned long long key = 0ull;
    auto load = [&](int, int, int i) -> c2 { return gsdr::pk::conj_mul(x[i], c[i]); };
    auto store = [&](int i, c2 v, int) {
        const float m = __builtin_fmaf(v.x, v.x, v.y * v.y);
        const unsigned long long k = ((unsigned long long)__float_as_uint(m) << 32) | (0xffffffffu - (uint32_t)i);
        key = k > key ? k : key;
    };
    MP::template run<false>(lds, tw, load, store, [] {});
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        {
            const unsigned long long o = __shfl_xor(key, off);
            key = o > key ? o : key;
        }
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        {
#pragma unroll
            for (int w = 1; w < NW; ++w) key = scratch[w] > key ? scratch[w] : key;
            const uint32_t idx = 0xffffffffu - (uint32_t)(key & 0xffffffffu);
            res[bp].code_phase = idx;
            res[bp].acq_delay_samples = (double)fmodf((float)idx, samples_per_code);
            if constexpr (PEAK)
                {
                    const float peak = __uint_as_float((uint32_t)(key >> 32));
                    res[bp].peak = peak;
                    // step two's statistic, which acq_reduce_kernel formed from the row maximum
                    // (the first step's is formed below, the peak ratio's by the second-peak pass)
                    if (ap.cfar && ap.step_two)
                        {
                            const float stat = peak / res[bp].input_power;
                            res[bp].test_statistic = stat;
                            res[bp].positive = stat > ap.threshold ? 1 : 0;
                        }
                }
        }
    if constexpr (STAT >= 2)
        {
            // CFAR input power of the row opposite the peak (pcps_acquisition.cc:531-533)
            // by Parseval: accumulate(|R|^2) / fft_size = sum_k |X_opp[k]|^2 |C[k]|^2
            if (!ap.cfar || ap.step_two) return;
            const uint32_t opp = (d + D / 2) % D;
            const c2* xo = reinterpret_cast<const c2*>(X) + ap.xm.off(b, opp);
            float acc = 0.0f;
            for (uint32_t i = threadIdx.x; i < N; i += NT)
                {
                    const c2 y = gsdr::pk::conj_mul(xo[i], c[i]);
                    acc = __builtin_fmaf(y.x, y.x, __builtin_fmaf(y.y, y.y, acc));
                }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            float* fs = reinterpret_cast<float*>(scratch + NW);
            __syncthreads();
            if ((threadIdx.x & 63) == 0) fs[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0)
                {
                    float tot = 0.0f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) tot += fs[w];
                    // (float)((double)(acc / eff) / 2.0 / counter), acc / eff = tot
                    const float ip = (float)((double)tot / 2.0 / (double)ap.counter);
                    gsdr_acq_result r = res[bp];
                    r.input_power = ip;
                    r.test_statistic = r.peak / ip;
                    r.positive = r.test_statistic > ap.threshold ? 1 : 0;
                    res[bp] = r;
                }
        }
}

// ---------------------------------------------------------------- general path (dwells, bit transition)
// acquisition_core with max_dwells K > 1 (non-coherent accumulation of |R|^2 over
// K consecutive blocks, pcps_acquisition.cc:667-675) and/or bit_transition_flag
// (outputs [N/2, N) of each transform, :671).  One workgroup per (attempt b, d, p)
// runs the K transforms of dwells k = 0..K-1 (blocks b*K + k); each lane adds |R|^2
// into its own entries of a pooled global row (every plan maps an output index to
// the same lane in every transform, so no synchronisation is needed) and row
// statistics of the accumulated grid are emitted after every dwell:
// stats[((b*P + p)*K + k)*D + d].
__device__ __forceinline__ int pool_acquire(uint32_t* slots, int nwords)
{
    __shared__ int s_slot;
    if (threadIdx.x == 0)
        {
            int w = (int)((blockIdx.x + blockIdx.y * gridDim.x) % (unsigned)nwords);
            for (;;)
                {
                    const uint32_t cur = __hip_atomic_load(&slots[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur != 0xffffffffu)
                        {
                            const int bit = __builtin_ctz(~cur);
                            const uint32_t old =
                                __hip_atomic_fetch_or(&slots[w], 1u << bit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                            if (!(old & (1u << bit)))
                                {
                                    s_slot = w * 32 + bit;
                                    break;
                                }
                        }
                    else
                        {
                            w = w + 1 == nwords ? 0 : w + 1;
                            __builtin_amdgcn_s_sleep(2);
                        }
                }
        }
    __syncthreads();
    return s_slot;
}

__device__ __forceinline__ void pool_release(uint32_t* slots, int slot)
{
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_and(&slots[slot >> 5], ~(1u << (slot & 31)), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// Cell (b, d, p) of a 1-D correlate grid over nrows = nblocks * D rows x P PRNs,
// XCD-aware for code reuse: workgroup ids go to the XCDs round-robin, so XCD x
// takes rows x, x + 8, ... and walks them PRN-group-major -- for each group of PG
// PRNs (PG | P) every one of its rows, the group's PG transforms of a row
// consecutively.  An XCD's L2 then holds PG code spectra while the X rows stream
// (at C4, N = 64000: 4 x 512 KB of codes instead of cycling through all 36) and
// each X row is fetched once per group.  Rows beyond the last multiple of 8 are
// mapped row-major.
__device__ __forceinline__ void dwell_cell(uint32_t D, uint32_t P, uint32_t nrows, uint32_t& b, uint32_t& d,
    uint32_t& p)
{
    const uint32_t id = blockIdx.x;
    const uint32_t full = nrows >> 3;
    const uint32_t PG = (P % 4u == 0u) ? 4u : ((P % 2u == 0u) ? 2u : 1u);
    uint32_t row;
    if (id < full * 8u * P)
        {
            const uint32_t xcd = id & 7u, slot = id >> 3;
            const uint32_t per_group = full * PG;
            const uint32_t pg = slot / per_group, rem = slot - pg * per_group;
            const uint32_t ri = rem / PG;
            row = ri * 8u + xcd;
            p = pg * PG + (rem - ri * PG);
        }
    else
        {
            const uint32_t t = id - full * 8u * P;
            row = full * 8u + t / P;
            p = t - (t / P) * P;
        }
    b = row / D;
    d = row - b * D;
}

template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_correlate_dwell_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap, float* __restrict__ acc_pool, uint32_t* __restrict__ acc_slots,
    int acc_words)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    const uint32_t N = plan.n;
    uint32_t b, d, p;
    dwell_cell(ap.D, ap.P, gridDim.x / ap.P, b, d, p);
    const uint32_t K = ap.dwells;
    const int slot = K > 1 ? pool_acquire(acc_slots, acc_words) : 0;
    float* acc = acc_pool + (size_t)slot * ap.eff;
    const float2* c = code_fft + (size_t)p * N;
    for (uint32_t k = 0; k < K; ++k)
        {
            const float2* x = X + ap.xm.off(b * K + k, d);
            float best = -1.0f, sum = 0.0f;
            uint32_t bidx = 0xffffffffu;
            auto load = [&](int i) -> float2 {
                float2 a = x[i], q = c[i];
                return make_float2(a.x * q.x + a.y * q.y, a.x * q.y - a.y * q.x);
            };
            auto store = [&](int i, float2 v) {
                const int j = i - (int)ap.out_off;
                if (j < 0) return;
                float m = v.x * v.x + v.y * v.y;
                if (K > 1)
                    {
                        if (k > 0) m = acc[j] + m;  // volk_32f_x2_add_32f(grid, grid, tmp)
                        acc[j] = m;
                    }
                if (stat_better(m, (uint32_t)j, best, bidx))
                    {
                        best = m;
                        bidx = (uint32_t)j;
                    }
                sum += m;
            };
            PT::run(plan, lds, tw, load, store);
            block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
            if (threadIdx.x == 0) stats[(((size_t)b * ap.P + p) * K + k) * ap.D + d] = RowStat{best, bidx, sum, 0};
        }
    if (K > 1) pool_release(acc_slots, slot);
}

// Peak-ratio statistic per dwell: the accumulated row d*_k over dwells 0..k,
// maximum outside the exclusion window (as acq_second_peak_kernel).  grid (K, B*P).
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_second_peak_dwell_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ resk, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap, float* __restrict__ acc_pool, uint32_t* __restrict__ acc_slots,
    int acc_words)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    const uint32_t kk = blockIdx.x, bp = blockIdx.y;
    const uint32_t K = ap.dwells;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t N = plan.n;
    gsdr_acq_result* rr = resk + (size_t)bp * K + kk;
    const uint32_t d = rr->doppler_index;
    const int32_t ti = (int32_t)rr->code_phase;
    // the reference wraps the exclusion window at d_fft_size even when the rows
    // hold the effective N/2 outputs (bit transition; :580-590)
    const int32_t E = (int32_t)ap.N;
    int32_t e1 = ti - (int32_t)ap.samples_per_chip;
    int32_t e2 = ti + (int32_t)ap.samples_per_chip;
    if (e1 < 0)
        e1 = E + e1;
    else if (e2 >= E)
        e2 = e2 - E;
    const int slot = kk > 0 ? pool_acquire(acc_slots, acc_words) : 0;
    float* acc = acc_pool + (size_t)slot * ap.eff;
    const float2* c = code_fft + (size_t)p * N;
    float best = 0.0f, sum = 0.0f;
    uint32_t bidx = 0;
    for (uint32_t k = 0; k <= kk; ++k)
        {
            const float2* x = X + ap.xm.off(b * K + k, d);
            const bool last = k == kk;
            auto load = [&](int i) -> float2 {
                float2 a = x[i], q = c[i];
                return make_float2(a.x * q.x + a.y * q.y, a.x * q.y - a.y * q.x);
            };
            auto store = [&](int i, float2 v) {
                const int j = i - (int)ap.out_off;
                if (j < 0) return;
                float m = v.x * v.x + v.y * v.y;
                if (kk > 0)
                    {
                        if (k > 0) m = acc[j] + m;
                        if (!last) acc[j] = m;
                    }
                if (last)
                    {
                        const bool excluded = (e1 < e2) ? (j >= e1 && j < e2) : (j >= e1 || j < e2);
                        if (excluded) m = 0.0f;
                        if (stat_better(m, (uint32_t)j, best, bidx))
                            {
                                best = m;
                                bidx = (uint32_t)j;
                            }
                    }
            };
            PT::run(plan, lds, tw, load, store);
        }
    block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
    if (threadIdx.x == 0)
        {
            gsdr_acq_result r = *rr;
            r.second_peak = best;
            r.test_statistic = r.peak / best;
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
            *rr = r;
        }
    if (kk > 0) pool_release(acc_slots, slot);
}

// ---------------------------------------------------------------- dwell per call (gsdr_acq_run_dwell)
// acquisition_core's own dwell loop: one call per general_work block, the |R|^2
// grid kept across calls (pcps_acquisition.cc:637-680: the first dwell writes
// d_magnitude_grid, later dwells add into it with volk_32f_x2_add_32f) in a
// device-resident grid[p][d][eff]; the statistic of the accumulated grid after
// every call (:689-696) with the dwell counter as the CFAR divisor (:534).
// One workgroup per (d, p) of one block.
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_dwell_grid_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap, float* __restrict__ grid, uint32_t dwell)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    const uint32_t N = plan.n;
    const uint32_t d = blockIdx.x / ap.P, p = blockIdx.x - d * ap.P;
    float* row = grid + ((size_t)p * ap.D + d) * ap.eff;
    const float2* x = X + ap.xm.off(0, d);
    const float2* c = code_fft + (size_t)p * N;
    float best = -1.0f, sum = 0.0f;
    uint32_t bidx = 0xffffffffu;
    auto load = [&](int i) -> float2 {
        float2 a = x[i], q = c[i];
        return make_float2(a.x * q.x + a.y * q.y, a.x * q.y - a.y * q.x);
    };
    auto store = [&](int i, float2 v) {
        const int j = i - (int)ap.out_off;
        if (j < 0) return;
        float m = v.x * v.x + v.y * v.y;
        if (dwell > 0) m = row[j] + m;
        row[j] = m;
        if (stat_better(m, (uint32_t)j, best, bidx))
            {
                best = m;
                bidx = (uint32_t)j;
            }
        sum += m;
    };
    PT::run(plan, lds, tw, load, store);
    block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
    if (threadIdx.x == 0) stats[(size_t)p * ap.D + d] = RowStat{best, bidx, sum, 0};
}

// ---------------------------------------------------------------- K_forward (packed f32)
// X_{b,d} = FFT(x_b .* w_d) on the packed plan (the N = 4000 path, with the packed
// correlate variants).  Grid (B, D) with the block index fastest, as
// acq_forward_kernel.
template <class MP, int IT>
__global__ void __launch_bounds__(MP::NT) acq_forward_pk_kernel(const void* __restrict__ iq, uint64_t block_stride,
    const float2* __restrict__ wipe, float2* __restrict__ X, const float2* __restrict__ tw, uint32_t consumed, XMap xm)
{
    using gsdr::pk::c2;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    const uint32_t b = blockIdx.x, d = blockIdx.y;
    constexpr uint32_t N = MP::N;
    const size_t base = (size_t)b * block_stride;
    const c2* w = reinterpret_cast<const c2*>(wipe) + (size_t)d * N;
    c2* out = reinterpret_cast<c2*>(X) + xm.off(b, d);
    const int ext = (int)(xm.stride - N);  // bins repeated after N - 1 (XMap)
    auto load = [&](int, int, int i) -> c2 {
        if (i >= (int)consumed) return c2{0.f, 0.f};
        return gsdr::pk::mul(gsdr::pk::from(load_item<IT>(iq, base + i)), w[i]);
    };
    auto store = [&](int i, c2 v, int) {
        out[i] = v;
        if (i < ext) out[N + i] = v;
    };
    MP::run(lds, tw, load, store, [] {});
}

// ---------------------------------------------------------------- K_second
// Peak-ratio statistic: recompute row d* of (b, p) and take the maximum outside
// the cyclic exclusion range [e1, e2) built as in pcps_acquisition.cc:580-604.
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_second_peak_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ res, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap)
{
    extern __shared__ float2 lds[];
    RowStat* scratch = reinterpret_cast<RowStat*>(lds + gsdr::fft::lds_elems_dev(plan));
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t N = plan.n;
    const uint32_t d = res[bp].doppler_index;
    const int32_t ti = (int32_t)res[bp].code_phase;
    // the window over the effective outputs j = i - out_off (bit transition: the
    // second half); the reference wraps it at d_fft_size all the same (:580-590)
    int32_t e1 = ti - (int32_t)ap.samples_per_chip;
    int32_t e2 = ti + (int32_t)ap.samples_per_chip;
    if (e1 < 0)
        e1 = (int32_t)N + e1;
    else if (e2 >= (int32_t)N)
        e2 = e2 - (int32_t)N;
    const float2* x = X + ap.xm.off(b, d);
    const float2* c = code_fft + (size_t)p * N;
    float best = 0.0f, sum = 0.0f;
    uint32_t bidx = 0;
    auto load = [&](int i) -> float2 {
        float2 a = x[i], k = c[i];
        return make_float2(a.x * k.x + a.y * k.y, a.x * k.y - a.y * k.x);
    };
    auto store = [&](int i, float2 v) {
        const int j = i - (int)ap.out_off;
        if (j < 0) return;
        const bool excluded = (e1 < e2) ? (j >= e1 && j < e2) : (j >= e1 || j < e2);
        const float m = excluded ? 0.0f : v.x * v.x + v.y * v.y;
        if (stat_better(m, (uint32_t)j, best, bidx))
            {
                best = m;
                bidx = (uint32_t)j;
            }
    };
    PT::run(plan, lds, tw, load, store);
    block_reduce_stat<PT::NT>(best, bidx, sum, scratch);
    if (threadIdx.x == 0)
        {
            gsdr_acq_result r = res[bp];
            r.second_peak = best;
            r.test_statistic = r.peak / best;
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
            res[bp] = r;
        }
}

// Peak ratio on the split path in one pass over the selected row: recompute row d*
// of (b, p) on PT once (acq_argmax_four_kernel + acq_second_peak_kernel recomputed
// it twice), keep its |R|^2 in the workgroup's row of rowbuf while finding the
// first maximum (index_max rule), then scan that row again for the maximum
// outside the exclusion window around it (pcps_acquisition.cc:580-604, wrapped at
// d_fft_size as the reference does).  Values bit-identical to the two kernels'.
template <class PT>
__global__ void __launch_bounds__(PT::NT) acq_argmax_second_four_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ res, const float2* __restrict__ tw,
    typename PT::PlanT plan, AcqParams ap, float* __restrict__ rowbuf)
{
    constexpr int NT = PT::NT;
    constexpr int NW = NT / 64;
    extern __shared__ float2 lds[];
    __shared__ unsigned long long s_key[NW];
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t N = ap.N;
    const uint32_t d = res[bp].doppler_index;
    if (d >= ap.D) return;  // uniform: no maximum found (an all-NaN grid)
    const float2* x = X + ap.xm.off(b, d);
    const float2* c = code_fft + (size_t)p * N;
    const int off = (int)ap.out_off;
    const uint32_t eff = N - (uint32_t)off;
    float* row = rowbuf + (size_t)bp * N;
    auto load = [&](int i) -> float2 {
        const float2 a = x[i], k = c[i];
        return make_float2(a.x * k.x + a.y * k.y, a.x * k.y - a.y * k.x);
    };
    unsigned long long key = 0ull;
    auto store = [&](int i, float2 v) {
        const int j = i - off;
        if (j < 0) return;
        const float m = __builtin_fmaf(v.x, v.x, v.y * v.y);
        row[j] = m;
        const unsigned long long k = ((unsigned long long)__float_as_uint(m) << 32) | (0xffffffffu - (uint32_t)j);
        key = k > key ? k : key;
    };
    PT::run(plan, lds, tw, load, store);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        {
            const unsigned long long t = __shfl_xor(key, o);
            key = t > key ? t : key;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_key[wave] = key;
    __syncthreads();  // also orders every lane's row stores before the scan below
#pragma unroll
    for (int w = 0; w < NW; ++w) key = s_key[w] > key ? s_key[w] : key;
    const uint32_t idx = 0xffffffffu - (uint32_t)(key & 0xffffffffu);
    const float peak = __uint_as_float((uint32_t)(key >> 32));
    // second peak (acq_second_peak_kernel's window and tie rule)
    const int32_t ti = (int32_t)idx;
    int32_t e1 = ti - (int32_t)ap.samples_per_chip;
    int32_t e2 = ti + (int32_t)ap.samples_per_chip;
    if (e1 < 0)
        e1 = (int32_t)N + e1;
    else if (e2 >= (int32_t)N)
        e2 = e2 - (int32_t)N;
    float best = 0.0f;
    uint32_t bidx = 0;
    for (uint32_t j = threadIdx.x; j < eff; j += NT)
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
    __syncthreads();  // s_key reuse
    unsigned long long k2 = ((unsigned long long)__float_as_uint(best) << 32) | (0xffffffffu - bidx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        {
            const unsigned long long t = __shfl_xor(k2, o);
            k2 = t > k2 ? t : k2;
        }
    if (lane == 0) s_key[wave] = k2;
    __syncthreads();
    if (threadIdx.x == 0)
        {
#pragma unroll
            for (int w = 0; w < NW; ++w) k2 = s_key[w] > k2 ? s_key[w] : k2;
            gsdr_acq_result r = res[bp];
            r.code_phase = idx;
            r.acq_delay_samples = (double)fmodf((float)idx, ap.samples_per_code);
            r.peak = peak;
            r.second_peak = __uint_as_float((uint32_t)(k2 >> 32));
            r.test_statistic = r.peak / r.second_peak;
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
            res[bp] = r;
        }
}

}  // namespace
