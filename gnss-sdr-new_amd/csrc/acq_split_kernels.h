// The register four-step (RegFourStep) and the correlate kernels built on it: one
// transform per workgroup (acq_correlate_reg_kernel, N = 16000) and the split family
// for the larger sizes.  Included only where they are instantiated (acq_pk.hip,
// acq_split.hip).
#pragma once
#include "acq_kernels.h"

namespace
{

// ---------------------------------------------------------------- K_correlate, register four-step
// For transforms whose full LDS image allows only one workgroup per CU (N = 16000
// at 16 Msps: 128 KB, so the workgroup's barriers and first-stage loads cannot
// overlap another's work).  N = R * L, decimation in frequency as in fft_4step.h:
//   phase 1: every lane takes CPL columns n2 of the R x L view, loads the R products
//            conj(X[n1 L + n2]) C[n1 L + n2] (coalesced), runs the packed DFT_R and
//            scales row k1 by W_N^{n2 k1} -- the whole transform now sits in VGPRs
//            (R * CPL complex per lane);
//   phase 2: R/H rounds: H rows go to LDS (H * L complex -- 64 KB for H = 8, L =
//            1000, so two workgroups share a CU), H batched L-point Stockham
//            transforms run there, the last stage's |.|^2 feeds the row maximum.
// Only the row maximum is kept (STAT 2): the outputs arrive in no particular order
// and duplicated (clamped) lanes only repeat values, which a maximum ignores.
// acq_argmax_pk_kernel recomputes the selected row on the full-LDS plan for the
// first-maximum index and the exact peak.
// Row layouts in LDS: row rw at rw * stride, element e at e + (e / S) * P -- one
// pad of P elements every S, so strided Stockham writes could spread over the banks.
// The stage functions need S | Ns (writes) and S | L/R (reads) so every address
// is a per-butterfly base plus a compile-time offset.  Pads chosen with an LDS bank
// model halved the measured bank conflicts of the 1000-point rows (0.30 -> 0.15 of
// the LDS-active cycles) and left the time unchanged -- the rows are VALU-issue bound
// (profiles/r05p) -- so every plan runs unpadded (NoPads).
template <int L, int S, int P>
struct RowPad
{
    static constexpr int stride = L + (S ? (L / S) * P : 0);
    static constexpr int pad_every = S;
    __device__ __forceinline__ static int pad(int e) { return S ? e + (e / S) * P : e; }
    static constexpr int cpad(int e) { return S ? e + (e / S) * P : e; }
};

template <int R, int NT, int L, int H, int Ns, bool LAST, class In, class OutL, class Out>
__device__ __forceinline__ void rows_stage(gsdr::pk::c2* lds, Out& out, int row0)
{
    using gsdr::pk::c2;
    constexpr int NB = L / R;       // butterflies per row
    constexpr int TOT = H * NB;     // butterflies of the stage
    constexpr int BPT = (TOT + NT - 1) / NT;
    constexpr int TSTRIDE = L / (Ns * R);
    // reads: element jb + r NB, pad(jb) + cpad(r NB) needs S | NB
    static_assert(In::pad_every == 0 || NB % In::pad_every == 0, "read layout: S must divide L/R");
    // writes: element (jb - k) R + k + r Ns (k < Ns), pad((jb - k) R) + k + cpad(r Ns)
    // needs S | Ns R and Ns | S
    static_assert(LAST || OutL::pad_every == 0 || ((Ns * R) % OutL::pad_every == 0 && OutL::pad_every % Ns == 0),
        "write layout: S must divide Ns R and be a multiple of Ns");
    const int wbase = (int)(threadIdx.x & ~63u);
    c2 v[BPT][R];
    int jb[BPT], rw[BPT];
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            const int jj = min((int)threadIdx.x + b * NT, TOT - 1);
            rw[b] = jj / NB;
            jb[b] = jj - rw[b] * NB;
            if (TOT % NT == 0 || wbase + b * NT < TOT)
                {
                    // element jb + r NB: the pad of r NB is compile-time (S | NB)
                    const int base = rw[b] * In::stride + In::pad(jb[b]);
#pragma unroll
                    for (int r = 0; r < R; ++r) v[b][r] = lds[base + In::cpad(r * NB)];
                }
        }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            if (TOT % NT == 0 || wbase + b * NT < TOT)
                {
                    int k = 0;
                    if constexpr (Ns > 1)
                        {
                            k = jb[b] % Ns;
                            gsdr::pk::apply_powers<R>(v[b], gsdr::pk::from(out.twiddle(k * TSTRIDE)));
                        }
                    gsdr::pk::Dft<R>::run(v[b]);
                    if constexpr (LAST)
                        {
#pragma unroll
                            for (int r = 0; r < R; ++r) out.value(v[b][r], jb[b] + r * Ns, row0 + rw[b]);  // row output jb + r Ns
                        }
                    else
                        {
                            // element (jb - k) R + k + r Ns: with S | Ns and S | Ns R the
                            // pad splits into the butterfly's part and a compile-time r part
                            const int base = rw[b] * OutL::stride + OutL::pad((jb[b] - k) * R) + k;
#pragma unroll
                            for (int r = 0; r < R; ++r) lds[base + OutL::cpad(r * Ns)] = v[b][r];
                        }
                }
        }
    if constexpr (!LAST) __syncthreads();
}

template <int NT, int L, int H, int Ns, class Pads, int Si, int R, int... Rest, class Out>
__device__ __forceinline__ void rows_stages(gsdr::pk::c2* lds, Out& out, int row0)
{
    constexpr bool LAST = sizeof...(Rest) == 0;
    using In = typename Pads::template layout<Si>;
    using OutL = typename Pads::template layout<LAST ? Si : Si + 1>;
    rows_stage<R, NT, L, H, Ns, LAST, In, OutL>(lds, out, row0);
    if constexpr (!LAST) rows_stages<NT, L, H, Ns * R, Pads, Si + 1, Rest...>(lds, out, row0);
}

// Pads for the buffers between the row stages (buffer 0 = phase 1's rows); a
// bank-model padding of the 1000-point rows measured within noise.
template <int L>
struct NoPads
{
    template <int I>
    using layout = RowPad<L, 0, 0>;
};

// ---- wave-local row transforms
// One wave transforms one L-point row in place in its own LDS row buffer: the
// Stockham exchange between the row stages needs no workgroup barrier, because
// a wave's LDS instructions execute in issue order -- every lane's reads of a
// stage are issued before any of its writes, and the next stage's reads after
// them.  The empty asm statements (memory clobber) keep the compiler from moving
// a write above a read whose address it believes distinct (other lanes' data is
// involved, which per-thread alias analysis cannot see).  Lanes past the stage's
// butterfly count repeat the last butterfly (same values to the same addresses,
// repeated outputs for an order-free maximum), so no lane is predicated off.
template <int R, int L, int Ns, bool LAST, class In, class OutL, class Out>
__device__ __forceinline__ void wl_stage(gsdr::pk::c2* row, Out& out, int lane, int k1)
{
    using gsdr::pk::c2;
    constexpr int NB = L / R;
    constexpr int BPT = (NB + 63) / 64;
    constexpr int TSTRIDE = L / (Ns * R);
    static_assert(In::pad_every == 0 || NB % In::pad_every == 0, "read layout: S must divide L/R");
    static_assert(LAST || OutL::pad_every == 0 || ((Ns * R) % OutL::pad_every == 0 && OutL::pad_every % Ns == 0),
        "write layout: S must divide Ns R and be a multiple of Ns");
    c2 v[BPT][R];
    int jb[BPT];
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            jb[b] = NB % 64 == 0 ? lane + 64 * b : min(lane + 64 * b, NB - 1);
            const int base = In::pad(jb[b]);
#pragma unroll
            for (int r = 0; r < R; ++r) v[b][r] = row[base + In::cpad(r * NB)];
        }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            int k = 0;
            if constexpr (Ns > 1)
                {
                    k = jb[b] % Ns;
                    gsdr::pk::apply_powers<R>(v[b], gsdr::pk::from(out.twiddle(k * TSTRIDE)));
                }
            gsdr::pk::Dft<R>::run(v[b]);
            if constexpr (LAST)
                {
#pragma unroll
                    for (int r = 0; r < R; ++r) out.value(v[b][r], jb[b] + r * Ns, k1);
                }
            else
                {
                    const int base = OutL::pad((jb[b] - k) * R) + k;
#pragma unroll
                    for (int r = 0; r < R; ++r) row[base + OutL::cpad(r * Ns)] = v[b][r];
                }
        }
    if constexpr (!LAST) asm volatile("" ::: "memory");
}

template <int L, int Ns, class Pads, int Si, int R, int... Rest, class Out>
__device__ __forceinline__ void wl_stages(gsdr::pk::c2* row, Out& out, int lane, int k1)
{
    constexpr bool LAST = sizeof...(Rest) == 0;
    using In = typename Pads::template layout<Si>;
    using OutL = typename Pads::template layout<LAST ? Si : Si + 1>;
    wl_stage<R, L, Ns, LAST, In, OutL>(row, out, lane, k1);
    if constexpr (!LAST) wl_stages<L, Ns * R, Pads, Si + 1, Rest...>(row, out, lane, k1);
}

// WPE_ packs the waves-per-EU hint (bits 0-3) and PGS (bits 4+): with PGS > 0 an
// XCD walks its rows PRN-group-major (groups of PGS PRNs, PGS | P), so its L2 holds
// PGS code spectra (PGS x 128 KB at N = 16000) instead of cycling through all P.
// H_ = 0: wave-local rows (WL): each round puts one row per wave in LDS and every
// wave transforms its own row without workgroup barriers (wl_stages); H = NT / 64
// rows per round, the last round partial when NT / 64 does not divide R.
template <int R_, int NT_, int H_, int WPE_, class Pads_, int... Rs>
struct RegFourStep
{
    static constexpr bool WL = H_ == 0;
    static constexpr int R = R_, NT = NT_, H = WL ? NT_ / 64 : H_, WPE = WPE_ & 15, PGS = WPE_ >> 4;
    static constexpr int L = (Rs * ...);
    static constexpr int N = R * L;
    static constexpr int CPL = (L + NT - 1) / NT;
    using Pads = Pads_;
    static constexpr int max_stride()
    {
        int m = L;
        constexpr int ns = sizeof...(Rs);
        if (ns > 1 && Pads::template layout<1>::stride > m) m = Pads::template layout<1>::stride;
        if (ns > 2 && Pads::template layout<2>::stride > m) m = Pads::template layout<2>::stride;
        if (ns > 3 && Pads::template layout<3>::stride > m) m = Pads::template layout<3>::stride;
        return m;
    }
    static constexpr int lds_elems = H * max_stride();
    static constexpr size_t lds_bytes() { return (size_t)lds_elems * sizeof(float2) + (NT / 64) * sizeof(float); }
    template <class Out>
    __device__ __forceinline__ static void row_transforms(gsdr::pk::c2* lds, Out& out, int row0)
    {
        rows_stages<NT, L, H, 1, Pads, 0, Rs...>(lds, out, row0);
    }
    // WL: one row (at lds, max_stride() elements) by the calling wave
    template <class Out>
    __device__ __forceinline__ static void wl_row(gsdr::pk::c2* row, Out& out, int lane, int k1)
    {
        wl_stages<L, 1, Pads, 0, Rs...>(row, out, lane, k1);
    }

    // Phase 2 of T register four-steps at once (LDS rounds of H rows): rows g = j R + k1
    // of transform j, so a round may hold rows of two transforms; out.value receives g
    // as the row index.  A last round with fewer than H rows leaves the rest of the LDS
    // rows stale: their outputs carry g >= T R, which out.value must drop.
    template <int T, int CPL, class Out>
    __device__ __forceinline__ static void phase2_multi(gsdr::pk::c2* lds, gsdr::pk::c2 (&v)[T][CPL][R], Out& out)
    {
        static_assert(!WL, "multi-transform phase 2: LDS rounds of H rows");
        const int wbase = (int)(threadIdx.x & ~63u);
#pragma unroll
        for (int h = 0; h < (T * R + H - 1) / H; ++h)
            {
                if (h > 0) __syncthreads();  // the previous round's last-stage reads are done
#pragma unroll
                for (int c = 0; c < CPL; ++c)
                    {
                        const int n2 = min((int)threadIdx.x + c * NT, L - 1);
                        if (L % NT == 0 || wbase + c * NT < L)
                            {
#pragma unroll
                                for (int i = 0; i < H; ++i)
                                    if (h * H + i < T * R) lds[i * L + n2] = v[(h * H + i) / R][c][(h * H + i) % R];
                            }
                    }
                __syncthreads();
                row_transforms(lds, out, h * H);
            }
    }
    // Phase 2 of a register four-step: the R rows (phase 1's v[c][k1], lane column
    // n2 = threadIdx.x + c NT, clamped) through LDS and the L-point row transforms.
    template <int CPL, class Out>
    __device__ __forceinline__ static void phase2(gsdr::pk::c2* lds, gsdr::pk::c2 (&v)[CPL][R], Out& out)
    {
        const int wbase = (int)(threadIdx.x & ~63u);
        auto column = [&](int c, int& n2) -> bool {
            n2 = min((int)threadIdx.x + c * NT, L - 1);
            return L % NT == 0 || wbase + c * NT < L;
        };
        if constexpr (!WL)
            {
                static_assert(R % H == 0, "rows go through LDS in groups of H");
#pragma unroll
                for (int h = 0; h < R / H; ++h)
                    {
                        if (h > 0) __syncthreads();  // the previous group's last-stage reads are done
#pragma unroll
                        for (int c = 0; c < CPL; ++c)
                            {
                                int n2;
                                if (column(c, n2))
                                    {
#pragma unroll
                                        for (int i = 0; i < H; ++i) lds[i * L + n2] = v[c][h * H + i];
                                    }
                            }
                        __syncthreads();
                        row_transforms(lds, out, h * H);
                    }
            }
        else
            {
                using L0 = typename Pads::template layout<0>;
                constexpr int STR = max_stride();
                const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
#pragma unroll
                for (int h = 0; h < (R + H - 1) / H; ++h)
                    {
                        if (h > 0) __syncthreads();  // every wave's row of the previous round is done
#pragma unroll
                        for (int c = 0; c < CPL; ++c)
                            {
                                int n2;
                                if (column(c, n2))
                                    {
#pragma unroll
                                        for (int i = 0; i < H; ++i)
                                            if (h * H + i < R) lds[i * STR + L0::pad(n2)] = v[c][h * H + i];
                                    }
                            }
                        __syncthreads();
                        if (h * H + wave < R) wl_row(lds + wave * STR, out, lane, h * H + wave);
                    }
            }
    }
};

template <class RP>
__global__ void __launch_bounds__(RP::NT) __attribute__((amdgpu_waves_per_eu(RP::WPE))) acq_correlate_reg_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, RowStat* __restrict__ stats, const float2* __restrict__ tw, uint32_t D,
    uint32_t P, uint32_t nblocks, XMap xm)
{
    using gsdr::pk::c2;
    constexpr int R = RP::R, NT = RP::NT, L = RP::L, CPL = RP::CPL;
    constexpr uint32_t N = RP::N;
    constexpr int NW = NT / 64;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    float* red = reinterpret_cast<float*>(lds_raw + RP::lds_elems);
    // (row = b*D + d, PRN p), XCD-aware: the P workgroups of one row on one XCD
    const uint32_t nrows = nblocks * D;
    const uint32_t id = blockIdx.x;
    const uint32_t full = nrows >> 3;
    uint32_t row, p;
    if (id < full * 8u * P)
        {
            const uint32_t xcd = id & 7u, slot = id >> 3;
            if (RP::PGS > 0 && P % (uint32_t)RP::PGS == 0)
                {
                    const uint32_t per_group = full * (uint32_t)RP::PGS;
                    const uint32_t pg = slot / per_group, rem = slot - pg * per_group;
                    const uint32_t ri = rem / (uint32_t)RP::PGS;
                    row = ri * 8u + xcd;
                    p = pg * (uint32_t)RP::PGS + (rem - ri * (uint32_t)RP::PGS);
                }
            else
                {
                    row = (slot / P) * 8u + xcd;
                    p = slot - (slot / P) * P;
                }
        }
    else
        {
            const uint32_t t = id - full * 8u * P;
            row = full * 8u + t / P;
            p = t - (t / P) * P;
        }
    const uint32_t b = row / D, d = row - (row / D) * D;
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(X) + xm.off(b, d), 0, (int)(N * sizeof(c2)), 0x00020000);
    const auto crs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(code_fft) + (size_t)p * N, 0, (int)(N * sizeof(c2)), 0x00020000);
    auto bload = [](decltype(xrs) rs, int voff, int soff) -> c2 {
        const auto u = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
        return c2{__uint_as_float(u[0]), __uint_as_float(u[1])};
    };
    const int wbase = (int)(threadIdx.x & ~63u);
    // phase 1: columns (clamped: a lane past L repeats column L-1, whose values
    // are written to the same LDS words and only repeat outputs)
    c2 v[CPL][R];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
        {
            if (L % NT == 0 || wbase + c * NT < L)
                {
                    const int n2 = min((int)threadIdx.x + c * NT, L - 1);
#pragma unroll
                    for (int n1 = 0; n1 < R; ++n1)
                        v[c][n1] = gsdr::pk::conj_mul(bload(xrs, n2 * 8, n1 * L * 8), bload(crs, n2 * 8, n1 * L * 8));
                    gsdr::pk::Dft<R>::run(v[c]);
                    gsdr::pk::apply_powers<R>(v[c], gsdr::pk::from(tw[n2]));
                }
        }
    struct Out
    {
        const float2* tw;
        float m;
        __device__ __forceinline__ float2 twiddle(int m_) const { return tw[m_ * R]; }  // W_L^m = W_N^{m R}
        __device__ __forceinline__ void value(c2 x, int, int) { m = __builtin_fmaxf(m, __builtin_fmaf(x.x, x.x, x.y * x.y)); }
    } out{tw, 0.0f};
    // phase 2: the rows k1 through LDS
    RP::phase2(lds, v, out);
    float rmax = gsdr::wave_max(out.m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = rmax;
    __syncthreads();
    if (threadIdx.x == 0)
        {
            float best = red[0];
#pragma unroll
            for (int w2 = 1; w2 < NW; ++w2) best = __builtin_fmaxf(best, red[w2]);
            stats[((size_t)b * P + p) * D + d] = RowStat{best, 0u, 0.0f, 0};
        }
}

// ---------------------------------------------------------------- K_correlate, split register four-step (large N)
// Transforms too large for one workgroup's registers (N = 64000: 512 KB, the whole
// register file of a CU; N = 100000) and the register-resident ones beyond the
// LDS engine (N = 25000, 32000).  Outer decimation in frequency by ROUT:
//   X[q + ROUT k'] = sum_m W_M^{m k'} z_q[m],   m < M = N / ROUT,
//   z_q[m] = W_N^{m q} sum_{r < ROUT} Y[r M + m] W_ROUT^{r q},
// so the ROUT sub-transforms own disjoint output sets and each one is a workgroup
// of its own: an M-point register four-step (phase 1 columns in VGPRs, phase 2
// rows through LDS, RegFourStep RP) whose loads form z_q from the ROUT products
// Y = conj(X) C of its input positions.  Nothing round-trips through a global
// scratch row (the packed four-step's phase-1 rows did, 2 x 8 N bytes per
// transform); a sub-transform re-reads the whole X and code rows instead, which
// the XCD-aware walk below keeps in L2.  Only the row maximum is kept (STAT 2,
// atomically merged over the ROUT sub-transforms); acq_argmax_four_kernel
// recomputes the selected row for the first-maximum index and the CFAR power.
// HALF (bit_transition_flag): only outputs k >= N / 2 are the reference's
// effective window (pcps_acquisition.cc:671); with k = q + ROUT (k1 + R k2),
// k >= N / 2 exactly when the row output k2 >= L / 2.
// Grid: one workgroup per (row = b*D + d, PRN p, sub-transform q), the ROUT*P
// workgroups of one row on one XCD, each XCD walking its rows in groups of pgs
// PRNs so its L2 holds pgs code rows while the X rows stream.
// ARG: the selected row's pass instead of the grid (acq_reduce_kernel chose Doppler
// row d* of (b, p) from the row maxima): grid (b*P + p, q), the same arithmetic as
// the grid pass (the recomputed values are bit-identical to those the row maximum
// came from), each output's key (|R|^2 bits, ~j) merged into keys[b*P + p] by a
// 64-bit atomic maximum -- the first maximum over the effective window j = k -
// (N - eff), index_max's rule (KERN/32f_index_max_32u.h:446-467) -- and, for the
// peak ratio, |R|^2 into the row's rowbuf entries; acq_argmax_split_finish_kernel
// turns the key into the result fields.  One workgroup per transform of a
// 100000-point row spreads the pass over ROUT x more CUs than the one-workgroup
// recomputation (acq_argmax_four_kernel: 144 workgroups at C5 Galileo).
// The input factor W_N^{m q} of sub-transform q is a compile-time root per column row
// and one table read per column (r04e: C4 bit transition +11 % over R reads).
// phase 1 staged through per-wave LDS rings (split_staged): the copies in flight per
// wave (2 KB of LDS each); 0: products straight from VGPR loads everywhere
#ifndef GSDR_SPLIT_DMA
#define GSDR_SPLIT_DMA 4
#endif
// the smallest outer radix staged (1: the 512-lane 25000 plan too), besides the
// one-column-per-lane plans, which are staged at any outer radix
#ifndef GSDR_SPLIT_DMA_MIN_ROUT
#define GSDR_SPLIT_DMA_MIN_ROUT 2
#endif
// waves per SIMD the staged grid pass is compiled for (4: <= 128 VGPRs, two 512-lane
// workgroups per CU as the VGPR form had)
#ifndef GSDR_SPLIT_WPE
#define GSDR_SPLIT_WPE 4
#endif
// staged phase 1's per-wave ring: slots of one X and PPW code copies (1 KB each per
// wave), as many in flight as GSDR_SPLIT_DMA allows within 144 KB per workgroup
template <class RP, int PPW>
struct SplitRing
{
    static constexpr int slot = 1024 * (1 + PPW);
    static constexpr int fit = 147456 / ((RP::NT / 64) * slot);
    static constexpr int depth = GSDR_SPLIT_DMA < fit ? GSDR_SPLIT_DMA : (fit > 0 ? fit : 1);
    static constexpr size_t bytes = (size_t)(RP::NT / 64) * depth * slot;
};

// which split plans stage phase 1 (r06, profiles/r06b3: 100000 = 4 x 25000 118 -> 133
// Msps, 64000 = 2 x 32000 88 -> 98, 32000 (one column per lane on 1024 lanes) 105 ->
// 118; the 512-lane 25000 plan, whose loads already go out 50 per column at once,
// 143 -> 138: left on VGPR loads)
template <int ROUT, class RP>
constexpr bool split_staged()
{
    return GSDR_SPLIT_DMA > 0 && (ROUT >= GSDR_SPLIT_DMA_MIN_ROUT || RP::CPL == 1);
}

// dynamic LDS of a split launch: phase 2's rows + the reduction slots (one float per
// wave and PRN of the workgroup: red[PPW * NW] after the rows) or, staged, each
// wave's ring of GSDR_SPLIT_DMA 2 KB copy slots, whichever is larger
template <int ROUT, class RP, int PPW = 1>
constexpr size_t split_lds_bytes()
{
    constexpr size_t ring = split_staged<ROUT, RP>() ? SplitRing<RP, PPW>::bytes : 0;
    constexpr size_t rows = RP::lds_bytes() + (size_t)(PPW - 1) * (RP::NT / 64) * sizeof(float);
    return ring > rows ? ring : rows;
}

template <int ROUT, class RP, bool HALF, bool ARG = false, int QPW = 1, int PPW = 1>
__global__ void __launch_bounds__(RP::NT) __attribute__((amdgpu_waves_per_eu(
    ARG ? 1 : (split_staged<ROUT, RP>() ? GSDR_SPLIT_WPE : RP::WPE)))) acq_correlate_split_kernel(
    const float2* __restrict__ X, const float2* __restrict__ code_fft, RowStat* __restrict__ stats,
    const float2* __restrict__ tw, uint32_t D, uint32_t P, uint32_t nblocks, uint32_t pgs, XMap xm,
    const gsdr_acq_result* __restrict__ sel, unsigned long long* __restrict__ keys, float* __restrict__ rowbuf,
    float* __restrict__ psum)
{
    using gsdr::pk::c2;
    constexpr int R = RP::R, NT = RP::NT, L = RP::L, CPL = RP::CPL;
    constexpr uint32_t M = RP::N;
    constexpr uint32_t N = M * ROUT;
    constexpr int NW = NT / 64;
    extern __shared__ float2 lds_raw[];
    c2* lds = reinterpret_cast<c2*>(lds_raw);
    float* red = reinterpret_cast<float*>(lds_raw + RP::lds_elems);
    static_assert(split_lds_bytes<ROUT, RP, PPW>() >= RP::lds_elems * sizeof(float2) + (size_t)PPW * NW * sizeof(float),
        "the launch's dynamic LDS covers red[PPW * NW]");
    // QPW sub-transforms per workgroup: q = qq + j RQ (j < QPW) -- they share every
    // product Y[r M + m] (only the exact outer factors W_ROUT^{r q} differ)
    static_assert(ROUT % QPW == 0 && (QPW == 1 || split_staged<ROUT, RP>()), "sub-transforms per workgroup");
    // or PPW PRNs per workgroup (ROUT 1): transform j correlates PRN p + j against the
    // same X row, read once for all of them
    static_assert(PPW == 1 || (ROUT == 1 && QPW == 1 && !ARG && PPW == 2 && split_staged<ROUT, RP>()),
        "PRNs per workgroup");
    constexpr int T = QPW * PPW;  // transforms per workgroup
    constexpr int RQ = ROUT / QPW;
    const uint32_t PV = P / PPW * RQ;  // virtual PRNs: pv = (p / PPW) RQ + qq
    const uint32_t nrows = nblocks * D;
    const uint32_t id = blockIdx.x;
    const uint32_t full = nrows >> 3;
    uint32_t row, pv;
    if constexpr (ARG)
        {
            const uint32_t bp = id / RQ;
            const uint32_t dsel = sel[bp].doppler_index;
            if (dsel >= D) return;  // uniform: no maximum found (an all-NaN grid)
            row = (bp / P) * D + dsel;
            pv = (bp - (bp / P) * P) * RQ + (id - bp * RQ);
        }
    else if (id < full * 8u * PV)
        {
            const uint32_t xcd = id & 7u, slot = id >> 3;
            const uint32_t G = pgs * RQ;  // PV % G == 0 (host)
            const uint32_t per_group = full * G;
            const uint32_t pg = slot / per_group, rem = slot - pg * per_group;
            const uint32_t ri = rem / G;
            row = ri * 8u + xcd;
            pv = pg * G + (rem - ri * G);
        }
    else
        {
            const uint32_t t = id - full * 8u * PV;
            row = full * 8u + t / PV;
            pv = t - (t / PV) * PV;
        }
    const uint32_t p = pv / RQ * PPW, q = pv - pv / RQ * RQ;  // q: the first sub-transform (qq); p the first PRN
    const uint32_t b = row / D, d = row - (row / D) * D;
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(X) + xm.off(b, d), 0, (int)(N * sizeof(c2)),
        0x00020000);
    const auto crs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float2*>(code_fft) + (size_t)p * N, 0, (int)(N * PPW * sizeof(c2)), 0x00020000);
    auto bload = [](decltype(xrs) rs, int voff, int soff) -> c2 {
        const auto u = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
        return c2{__uint_as_float(u[0]), __uint_as_float(u[1])};
    };
    const float2* xg = X + xm.off(b, d);
    const float2* cg = code_fft + (size_t)p * N;
    (void)xg;
    (void)cg;
    static_assert(ROUT == 1 || ROUT == 2 || ROUT == 4, "outer radix 1, 2 or 4");
    const int wbase = (int)(threadIdx.x & ~63u);
    // phase 1: columns (clamped lanes repeat column L-1), with the sub-transform
    // index q a compile-time constant: the outer factors W_ROUT^{rq} are exact
    // (+-1, +-i: an add/sub with swapped operands) and W_N^{mq} one table read
    // (m q < N)
    c2 v[T][CPL][R];
    // ROUT > 1: every element of a column sums ROUT products.  Loaded into VGPRs,
    // the compiler kept the accumulated columns resident and issued two loads and a
    // wait per product (r05: 200 dependent L2 round trips per column at 100000, VALU
    // issuing 29 % of the cycles).  Staged instead: each wave copies its own
    // columns' X and code values into its own LDS ring with global_load_lds
    // (dwordx4: one instruction moves two 512-byte segments -- one (row n1, quarter r,
    // column set c) each -- without VGPRs), DEPTH copies ahead of the products that
    // read them; no other wave reads a wave's ring, so no barrier, only its vmcnt.
    // Each element's sum keeps the r order (bit-identical).
    auto phase1_dma = [&](auto qc) {
        constexpr int Q = decltype(qc)::value;
        constexpr int DEPTH = SplitRing<RP, PPW>::depth, SLOT = SplitRing<RP, PPW>::slot;
        // segment s: column set c = s / U, unit u = s % U (n1 = u / ROUT, r = u % ROUT):
        // column-major, so a column's transform runs (and its registers settle) before
        // the next column accumulates, as in the VGPR form
        constexpr int U = R * ROUT;
        constexpr int PPC = (U + 1) / 2;          // copy pairs per column set (an odd U repeats its last unit)
        constexpr int PAIRS = PPC * CPL;         // one X and one code copy per two segments
        const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
        char* ring = reinterpret_cast<char*>(lds_raw) + (size_t)wave * DEPTH * SLOT;
        const int half = lane >> 5, l32 = lane & 31;
        const int lane_off = (wave * 64 + 2 * l32) * 8;
        auto issue = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < PAIRS)
                {
                    // lanes 0-31: unit 2kk of column set c, lanes 32-63: unit 2kk + 1 (an odd
                    // unit count repeats its last); two columns (16 B) per lane
                    constexpr int c = k / PPC, kk = k % PPC;
                    constexpr int ua = 2 * kk, ub = 2 * kk + 1 < U ? 2 * kk + 1 : 2 * kk;
                    constexpr int ea = (ua % ROUT) * (int)M + (ua / ROUT) * L + c * NT;
                    constexpr int eb = (ub % ROUT) * (int)M + (ub / ROUT) * L + c * NT;
                    // this lane's 16 bytes: the lane part in voffset, the first segment's
                    // element offset as the (uniform) scalar offset; bounds-checked buffer
                    // copies (lanes past column L - 1 copy bytes no lane reads, past the
                    // row's end zeros)
                    const int voff = lane_off + half * ((eb - ea) * 8);
                    char* dst = ring + (k % DEPTH) * SLOT;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (gsdr_lvoid*)dst, 16, voff, ea * 8, 0, 0);
#pragma unroll
                    for (int j = 0; j < PPW; ++j)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(crs, (gsdr_lvoid*)(dst + 1024 * (1 + j)), 16, voff,
                            (ea + j * (int)N) * 8, 0, 0);
                }
        };
        // the lane's column within its segment (clamped lanes read column L - 1's)
        int cl[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) cl[c] = min((int)threadIdx.x + c * NT, L - 1) - (c * NT + wave * 64);
        auto prologue = [&](auto kc) { issue(kc); };
        gsdr::pk::static_for<0, DEPTH>(prologue);
        auto step = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            // pair k has landed once at most (1 + PPW) (min(DEPTH, PAIRS - k) - 1) younger copies are out
            constexpr int younger = (1 + PPW) * ((PAIRS - k < DEPTH ? PAIRS - k : DEPTH) - 1);
            // s_waitcnt vmcnt(younger) (expcnt / lgkmcnt left at their maxima)
            __builtin_amdgcn_s_waitcnt((younger & 15) | (7 << 4) | (15 << 8) | ((younger >> 4) << 14));
            const char* src = ring + (k % DEPTH) * SLOT;
            auto seg = [&](auto jc) {
                constexpr int c = k / PPC, u = 2 * (k % PPC) + decltype(jc)::value;
                if constexpr (u < U)
                    {
                        constexpr int n1 = u / ROUT, r = u % ROUT;
                        if (L % NT == 0 || wbase + c * NT < L)
                            {
                                const int off = decltype(jc)::value * 512 + cl[c] * 8;
                                const c2 xv = *reinterpret_cast<const c2*>(src + off);
                                const c2 cv = *reinterpret_cast<const c2*>(src + 1024 + off);
                                const c2 y = gsdr::pk::conj_mul(xv, cv);
                                auto acc = [&](auto jq) {
                                    constexpr int J = decltype(jq)::value;
                                    constexpr int QJ = Q + (PPW == 1 ? J * RQ : 0);
                                    // W_ROUT^{r QJ} = W_4^{e}, e = (r QJ mod ROUT) * 4 / ROUT
                                    constexpr int e = ((r * QJ) % ROUT) * (4 / ROUT);
                                    c2& z = v[J][c][n1];
                                    if constexpr (PPW > 1 && J > 0)
                                        z = gsdr::pk::conj_mul(xv, *reinterpret_cast<const c2*>(src + 1024 * (1 + J) + off));
                                    else if constexpr (r == 0)
                                        z = y;
                                    else if constexpr (e == 0)
                                        z = z + y;
                                    else if constexpr (e == 1)
                                        z = gsdr::pk::add_mi(z, y);  // z + (-i) y
                                    else if constexpr (e == 2)
                                        z = z - y;
                                    else
                                        z = gsdr::pk::sub_mi(z, y);  // z + i y
                                    if constexpr (QJ > 0 && r == ROUT - 1) z = gsdr::pk::mul_root<QJ * n1, ROUT * R>(z);
                                };
                                gsdr::pk::static_for<0, T>(acc);
                            }
                    }
            };
            gsdr::pk::static_for<0, 2>(seg);
            // the slot's reads are done (their values are used above): refill it
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(std::integral_constant<int, k + DEPTH>{});
            // a column's last pair: its transform, while the next column's copies land
            // (fenced: interleaved with the next column's sums it spilled)
            if constexpr ((k + 1) % PPC == 0)
                {
                    constexpr int c = k / PPC;
                    __builtin_amdgcn_sched_barrier(0);
                    if (L % NT == 0 || wbase + c * NT < L)
                        {
                            const int n2 = min((int)threadIdx.x + c * NT, L - 1);
                            auto transform = [&](auto jq) {
                                constexpr int QJ = Q + (PPW == 1 ? decltype(jq)::value * RQ : 0);
                                c2(&w)[R] = v[decltype(jq)::value][c];
                                gsdr::pk::Dft<R>::run(w);
                                if constexpr (QJ > 0)
                                    {
                                        const c2 w0 = gsdr::pk::from(tw[QJ * n2]);
#pragma unroll
                                        for (int k1 = 0; k1 < R; ++k1) w[k1] = gsdr::pk::mul(w[k1], w0);
                                    }
                                gsdr::pk::apply_powers<R>(w, gsdr::pk::from(tw[ROUT * n2]));
                                __builtin_amdgcn_sched_barrier(0);
                            };
                            gsdr::pk::static_for<0, T>(transform);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
        };
        gsdr::pk::static_for<0, PAIRS>(step);
        // phase 2 writes rows over the rings: every wave's reads are done first
        __syncthreads();
    };
    auto phase1 = [&](auto qc) {
        constexpr int Q = decltype(qc)::value;
        if constexpr (split_staged<ROUT, RP>())
            {
                phase1_dma(qc);
                return;
            }
#pragma unroll
        for (int c = 0; c < CPL; ++c)
            {
                if (L % NT == 0 || wbase + c * NT < L)
                    {
                        const int n2 = min((int)threadIdx.x + c * NT, L - 1);
                        auto column_input = [&](auto n1c) {
                                constexpr int n1 = decltype(n1c)::value;
                                const int m = n1 * L + n2;
                                (void)m;
                                c2 z = gsdr::pk::conj_mul(bload(xrs, n2 * 8, n1 * L * 8), bload(crs, n2 * 8, n1 * L * 8));
#pragma unroll
                                for (int r = 1; r < ROUT; ++r)
                                    {
                                        const int so = (int)((r * M + n1 * L) * 8);
                                        const c2 y = gsdr::pk::conj_mul(bload(xrs, n2 * 8, so), bload(crs, n2 * 8, so));
                                        // W_ROUT^{r Q} = W_4^{e}, e = (r Q mod ROUT) * 4 / ROUT
                                        const int e = ((r * Q) % ROUT) * (4 / ROUT);
                                        if (e == 0)
                                            z = z + y;
                                        else if (e == 1)
                                            z = gsdr::pk::add_mi(z, y);  // z + (-i) y
                                        else if (e == 2)
                                            z = z - y;
                                        else
                                            z = gsdr::pk::sub_mi(z, y);  // z + i y
                                    }
                                if constexpr (Q > 0) z = gsdr::pk::mul_root<Q * n1, ROUT * R>(z);
                                v[0][c][n1] = z;
                        };
                        gsdr::pk::static_for<0, R>(column_input);
                        gsdr::pk::Dft<R>::run(v[0][c]);
                        // W_M^{n2 k1} = W_N^{ROUT n2 k1}; the input factor W_N^{m Q} =
                        // W_{ROUT R}^{Q n1} W_N^{Q n2} -- the first a compile-time root
                        // above, the second common to the column, so applied to its
                        // outputs here: one table read instead of R
                        if constexpr (Q > 0)
                            {
                                const c2 w0 = gsdr::pk::from(tw[Q * n2]);
#pragma unroll
                                for (int k1 = 0; k1 < R; ++k1) v[0][c][k1] = gsdr::pk::mul(v[0][c][k1], w0);
                            }
                        gsdr::pk::apply_powers<R>(v[0][c], gsdr::pk::from(tw[ROUT * n2]));
                    }
            }
    };
    auto run_phase1 = [&](auto qc) { phase1(qc); };
    if constexpr (RQ == 1)
        run_phase1(std::integral_constant<int, 0>{});
    else if constexpr (RQ == 2)
        {
            if (q == 0)
                run_phase1(std::integral_constant<int, 0>{});
            else
                run_phase1(std::integral_constant<int, 1>{});
        }
    else
        {
            switch (q)
                {
                case 0: run_phase1(std::integral_constant<int, 0>{}); break;
                case 1: run_phase1(std::integral_constant<int, 1>{}); break;
                case 2: run_phase1(std::integral_constant<int, 2>{}); break;
                default: run_phase1(std::integral_constant<int, 3>{}); break;
                }
        }
    struct Out
    {
        const float2* tw;
        float m;
        unsigned long long key;
        float* row;  // ARG with the peak ratio: the row's |R|^2 (effective window)
        uint32_t q;
        float m1;  // PPW 2: the second PRN's row maximum
        // W_L^m = W_N^{m R ROUT}
        __device__ __forceinline__ float2 twiddle(int m_) const { return tw[m_ * R * ROUT]; }
        // g: the row (k1 of transform g / R, g mod R: sub-transform q + (g / R) RQ, or PRN
        // p + g / R with PPW)
        __device__ __forceinline__ void value(c2 x, int k2, int g)
        {
            const float a = __builtin_fmaf(x.x, x.x, x.y * x.y);
            if (HALF && k2 < L / 2) return;
            if constexpr (!RP::WL && (T * R) % RP::H != 0)
                {
                    if (g >= T * R) return;  // a stale row of a partial last round
                }
            if constexpr (ARG)
                {
                    const uint32_t k1 = (uint32_t)g % (uint32_t)R, qo = q + ((uint32_t)g / (uint32_t)R) * (uint32_t)RQ;
                    // output k = qo + ROUT (k1 + R k2); effective index j = k - (N - eff)
                    const uint32_t j = qo + (uint32_t)ROUT * (k1 + (uint32_t)R * (uint32_t)k2) - (HALF ? N / 2 : 0u);
                    const unsigned long long kk = ((unsigned long long)__float_as_uint(a) << 32) | (0xffffffffu - j);
                    key = kk > key ? kk : key;
                    if (row) row[j] = a;
                }
            else if constexpr (PPW > 1)
                {
                    if (g < R)
                        m = __builtin_fmaxf(m, a);
                    else
                        m1 = __builtin_fmaxf(m1, a);
                }
            else
                m = __builtin_fmaxf(m, a);
        }
    } out{tw, 0.0f, 0ull, nullptr, q, 0.0f};
    if constexpr (ARG)
        {
            if (rowbuf) out.row = rowbuf + (size_t)(id / RQ) * (HALF ? N / 2 : N);
        }
    if constexpr (T == 1 && (RP::WL || RP::R % RP::H == 0))
        RP::template phase2<CPL>(lds, v[0], out);
    else
        RP::template phase2_multi<T, CPL>(lds, v, out);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (ARG)
        {
            unsigned long long k = out.key;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                {
                    const unsigned long long t = __shfl_xor(k, o);
                    k = t > k ? t : k;
                }
            unsigned long long* sk = reinterpret_cast<unsigned long long*>(lds_raw);
            __syncthreads();  // every wave's phase-2 LDS reads are done: reuse the row buffer
            if (lane == 0) sk[wave] = k;
            __syncthreads();
            if (threadIdx.x == 0)
                {
#pragma unroll
                    for (int w2 = 1; w2 < NW; ++w2) k = sk[w2] > k ? sk[w2] : k;
                    __hip_atomic_fetch_max(&keys[id / RQ], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            if (psum)
                {
                    // CFAR: this sub-transform's share of the Parseval sum of the row
                    // opposite the peak (pcps_acquisition.cc:531-533): sum |conj(X_opp) C|^2
                    // over inputs [q M, (q + 1) M), lane-strided, then wave and workgroup
                    // sums in a fixed order; the finish kernel adds the ROUT shares in q order
                    const uint32_t bp = id / RQ;
                    const uint32_t opp = (d + D / 2) % D;
                    float* sf = reinterpret_cast<float*>(sk + NW);
#pragma unroll
                    for (int jq = 0; jq < QPW; ++jq)
                        {
                            const uint32_t qo = q + (uint32_t)jq * RQ;
                            const c2* xo = reinterpret_cast<const c2*>(X) + xm.off(b, opp) + (size_t)qo * M;
                            const c2* co = reinterpret_cast<const c2*>(code_fft) + (size_t)p * N + (size_t)qo * M;
                            float acc = 0.0f;
                            for (uint32_t i = threadIdx.x; i < M; i += NT)
                                {
                                    const c2 y = gsdr::pk::conj_mul(xo[i], co[i]);
                                    acc = __builtin_fmaf(y.x, y.x, __builtin_fmaf(y.y, y.y, acc));
                                }
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                            if (jq > 0) __syncthreads();  // thread 0 read the previous share's slots
                            if (lane == 0) sf[wave] = acc;
                            __syncthreads();
                            if (threadIdx.x == 0)
                                {
                                    float tot = 0.0f;
#pragma unroll
                                    for (int w2 = 0; w2 < NW; ++w2) tot += sf[w2];
                                    psum[(size_t)bp * ROUT + qo] = tot;
                                }
                        }
                }
            return;
        }
    float rmax = gsdr::wave_max(out.m);
    if (lane == 0) red[wave] = rmax;
    if constexpr (PPW > 1)
        {
            const float rmax1 = gsdr::wave_max(out.m1);
            if (lane == 0) red[NW + wave] = rmax1;
        }
    __syncthreads();
    if constexpr (PPW > 1)
        {
            if (threadIdx.x == 0)
                {
                    float best1 = red[NW];
#pragma unroll
                    for (int w2 = 1; w2 < NW; ++w2) best1 = __builtin_fmaxf(best1, red[NW + w2]);
                    stats[((size_t)b * P + p + 1) * D + d] = RowStat{best1, 0u, 0.0f, 0};
                }
        }
    if (threadIdx.x == 0)
        {
            float best = red[0];
#pragma unroll
            for (int w2 = 1; w2 < NW; ++w2) best = __builtin_fmaxf(best, red[w2]);
            RowStat* st = stats + ((size_t)b * P + p) * D + d;
            if constexpr (ROUT == 1)
                *st = RowStat{best, 0u, 0.0f, 0};
            else  // non-negative floats order as their bit patterns (row zeroed by the host)
                __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(&st->max), __float_as_uint(best), __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
        }
}

// The selected rows' results from acq_correlate_split_kernel<ARG>'s keys: code
// phase, Acq_delay_samples = fmod(indext, samples_per_code) (pcps_acquisition.cc:709)
// and the peak from the key; CFAR: the input power of the row opposite the peak by
// Parseval (:531-533, as acq_argmax_four_kernel over the whole row, same summation
// order); peak ratio: the second peak outside the +-1 chip window around the first
// (:580-604, wrapped at d_fft_size as the reference does) from the rowbuf row.
// One 256-lane workgroup per (b, p).  Not for CFAR with bit transition (the
// opposite row's half window needs its transform: acq_argmax_four_kernel).
template <int NT>
__global__ void __launch_bounds__(NT) acq_argmax_split_finish_kernel(const float2* __restrict__ X,
    const float2* __restrict__ code_fft, gsdr_acq_result* __restrict__ res, const unsigned long long* __restrict__ keys,
    const float* __restrict__ rowbuf, const float* __restrict__ psum, uint32_t nps, AcqParams ap)
{
    constexpr int NW = NT / 64;
    __shared__ unsigned long long s_key[NW];
    __shared__ float s_sum[NW];
    const uint32_t bp = blockIdx.x;
    const uint32_t b = bp / ap.P, p = bp - b * ap.P;
    const uint32_t N = ap.N;
    const uint32_t d = res[bp].doppler_index;
    if (d >= ap.D) return;  // uniform
    const unsigned long long key = keys[bp];
    const uint32_t idx = 0xffffffffu - (uint32_t)(key & 0xffffffffu);
    const float peak = __uint_as_float((uint32_t)(key >> 32));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ip = 0.0f, second = 0.0f;
    if (ap.cfar && !ap.step_two && psum)
        {
            // the split pass's per-sub-transform shares, in sub-transform order
            float tot = 0.0f;
            for (uint32_t i = 0; i < nps; ++i) tot += psum[(size_t)bp * nps + i];
            ip = (float)((double)tot / 2.0 / (double)ap.counter);
        }
    else if (ap.cfar && !ap.step_two)
        {
            const uint32_t opp = (d + ap.D / 2) % ap.D;
            const float2* xo = X + ap.xm.off(b, opp);
            const float2* c = code_fft + (size_t)p * N;
            float acc = 0.0f;
            for (uint32_t i = threadIdx.x; i < N; i += NT)
                {
                    const float2 a = xo[i], k = c[i];
                    const float yr = a.x * k.x + a.y * k.y, yi = a.x * k.y - a.y * k.x;
                    acc = __builtin_fmaf(yr, yr, __builtin_fmaf(yi, yi, acc));
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) s_sum[wave] = acc;
            __syncthreads();
            float tot = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += s_sum[w];
            ip = (float)((double)tot / 2.0 / (double)ap.counter);
        }
    else if (!ap.cfar)
        {
            const uint32_t eff = ap.eff;
            const float* row = rowbuf + (size_t)bp * eff;
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
            unsigned long long k2 = ((unsigned long long)__float_as_uint(best) << 32) | (0xffffffffu - bidx);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                {
                    const unsigned long long t = __shfl_xor(k2, o);
                    k2 = t > k2 ? t : k2;
                }
            if (lane == 0) s_key[wave] = k2;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) k2 = s_key[w] > k2 ? s_key[w] : k2;
            second = __uint_as_float((uint32_t)(k2 >> 32));
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
                }
            else
                {
                    r.second_peak = second;
                    r.test_statistic = r.peak / r.second_peak;
                }
            r.positive = r.test_statistic > ap.threshold ? 1 : 0;
            res[bp] = r;
        }
}

}  // namespace
