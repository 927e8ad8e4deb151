// Tracking: the correlator of one call -- sample sources, replica gathers and the
// E/P/L dot products, from the LDS window, HBM or the streamed chunk buffers.
#pragma once
#include "fft_pk.h"
#include "gsdr_internal.h"
#include "trk_types.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

namespace
{
using namespace gsdr::trk;

struct Prep  // lane-0 -> workgroup broadcast of one call's NCO
{
    double psi0, theta;
    float2 wstep;
    float rem_code, code_step;
    int64_t off;
    int32_t go;
    int32_t woff;  // >= 0: this call's samples are in the LDS window at that offset
    int32_t wrap;  // code index range of the call: 2 within the replica's margins, 1 within [-L, 2L), 0 general
    int32_t narrow;  // the call uses the narrow tap shifts
    int32_t pf_ok;   // streamed call: chunk 0 is in the buffer prefetched during the previous update
    // high_dyn: rotator rate term and resampler rate (do_correlation_step, :1069-1075),
    // taps 1..K-1 as sample-shifted copies of tap 0 (32f_xn_high_dynamics_resampler_32f_xn.h:84-91)
    int32_t hd;
    double theta_rate;
    float code_rate;
    int32_t hdshift[kMaxTrkTaps];
};

template <int IT>
__device__ __forceinline__ float2 load_iq(const void* __restrict__ p, int64_t i)
{
    if constexpr (IT == GSDR_ITEM_GR_COMPLEX)
        return reinterpret_cast<const float2*>(p)[i];
    else if constexpr (IT == GSDR_ITEM_CSHORT)
        {
            const short2 s = reinterpret_cast<const short2*>(p)[i];
            return make_float2((float)s.x, (float)s.y);
        }
    else
        {
            // Ibyte_To_Complex: interleaved_char_to_complex, scale 1 (exact)
            const char2 s = reinterpret_cast<const char2*>(p)[i];
            return make_float2((float)s.x, (float)s.y);
        }
}

__device__ __forceinline__ int wrap_code(int raw, int L)
{
    if (raw < 0) raw += L;
    if (raw >= L) raw -= L;
    if ((unsigned)raw >= (unsigned)L)
        {
            raw %= L;
            if (raw < 0) raw += L;
        }
    return raw;
}

template <int IT>
constexpr int item_bytes()
{
    return IT == GSDR_ITEM_GR_COMPLEX ? 8 : (IT == GSDR_ITEM_CSHORT ? 4 : 2);
}

// one stream item from an LDS byte image of the input (raw item format)
template <int IT>
__device__ __forceinline__ float2 lds_iq(const char* b, int byte)
{
    if constexpr (IT == GSDR_ITEM_GR_COMPLEX)
        return *reinterpret_cast<const float2*>(b + byte);
    else if constexpr (IT == GSDR_ITEM_CSHORT)
        {
            const short2 v = *reinterpret_cast<const short2*>(b + byte);
            return make_float2((float)v.x, (float)v.y);
        }
    else
        {
            const char2 v = *reinterpret_cast<const char2*>(b + byte);
            return make_float2((float)v.x, (float)v.y);
        }
}

// Asynchronous copy of input bytes [first, first + nbytes) (relative to the
// stream pointer) into an LDS buffer with global_load_lds_dwordx4: no VGPR
// destinations, so a whole chunk is in flight at once.  The buffer starts at the
// 16-byte block holding `first` (returned); every lane's source is clamped to a
// 16-byte block holding at least one byte of the stream, i.e. inside the
// stream's own pages.  Waves [w0, kTrkThreads/64) issue; the buffer is valid
// after the issuing waves' vmcnt drains: each issuing wave runs s_waitcnt
// vmcnt(0) before the barrier that hands the buffer over (correlate_call_stream).
__device__ __forceinline__ uintptr_t stream_fetch(const void* iq, uint64_t iq_bytes, int64_t first, int nbytes,
    char* lds, int w0)
{
    const uintptr_t base = reinterpret_cast<uintptr_t>(iq);
    const uintptr_t lo = base & ~(uintptr_t)15;
    const uintptr_t hi = (base + iq_bytes - 1) & ~(uintptr_t)15;
    const uintptr_t start = (uintptr_t)((int64_t)base + first) & ~(uintptr_t)15;
    const int rows = (nbytes + 15 + kStreamRow - 1) / kStreamRow;  // first - start <= 15
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    for (int r = wave - w0; r < rows; r += kTrkThreads / 64 - w0)
        {
            if (r < 0) break;
            uintptr_t a = start + (uintptr_t)r * kStreamRow + (uintptr_t)lane * 16;
            a = a < lo ? lo : (a > hi ? hi : a);
            __builtin_amdgcn_global_load_lds((gsdr_gvoid*)a, (gsdr_lvoid*)(lds + r * kStreamRow), 16, 0, 0);
        }
    return start;
}

// the two f16 halves of a compact replica word (gathered as float bits), widened (exact)
__device__ __forceinline__ float half_lo(float w)
{
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(__float_as_uint(w) & 0xffffu));
}
__device__ __forceinline__ float half_hi(float w)
{
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(__float_as_uint(w) >> 16));
}

// (int)floorf(x) in one instruction (v_cvt_flr_i32_f32: floor, then convert; exact)
__device__ __forceinline__ int floor_i(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// The plan values every chunk of a call uses, in SGPRs: read from the LDS plan once
// per call.  Read per chunk, behind the streamed calls' barriers, their wait also
// waited for the chunk's own sample loads.
struct ChunkNco
{
    float cstep, wsx, wsy;
    int wrap;
};
__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ ChunkNco chunk_nco(const Prep& p)
{
    return ChunkNco{uniform_f(p.code_step), uniform_f(p.wstep.x), uniform_f(p.wstep.y),
        __builtin_amdgcn_readfirstlane(p.wrap)};
}

// One correlation chunk of SPL (<= kSpl) samples per lane (n = n0 + tid +
// j*kTrkThreads), KT taps, no branches inside.  FULL: every sample of the chunk lies inside the
// call; otherwise samples past the end are zero and their index clamped.
// WRAP: 2 = every code index of the call lies in [-kCodeMargin, L + kCodeMargin),
// read straight from the margin-padded replica; 1 = in [-L, 2L), one conditional
// add/sub; 0 = general modulo.  Complex products and the accumulations are
// packed-f32 (v_pk_mul/v_pk_fma: one instruction per tap and sample).
// DATA: one more accumulator, acc[kMaxTrkTaps], on the data-component replica
// s_data at the prompt tap's index (the pilot-tracking data correlator of
// do_correlation_step, whose only tap sits at the prompt shift).
// PACK: the compact replica (pilot tracking of the 10230-chip signals): one LDS
// word per code index, the pilot chip as an f16 in its low half and the data
// chip in its high half (s_code points at the words, s_data is unused).  The
// data chip comes out of the prompt tap's word, so the call has no data gather;
// each gathered word costs one v_cvt_f32_f16 more (KT + 1 per sample).  The host
// packs only values an f16 holds exactly, so the converted floats, the FMAs and
// the sums are those of the float layout.
template <int IT, int SRC, int WRAP, bool FULL, int KT, bool DATA, int SPL = kSpl, bool PACK = false>
__device__ __forceinline__ void correlate_chunk(const void* __restrict__ iq, const float2* s_win, const float* s_code,
    const float* s_data, const Prep& p, const ChunkNco& q, int n0, int vl, int L, const float (&sh_rem)[kMaxTrkTaps], float2& ph,
    float2 (&acc)[kMaxTrkTaps + 1], const char* sbuf = nullptr, int sboff = 0)
{
    using gsdr::pk::c2;
    constexpr int IPK = KT / 2;  // prompt slot: 1 of E,P,L / 2 of VE,E,P,L,VL
    // Five phases, fenced so the scheduler keeps them apart: (1) the samples (LDS
    // or HBM) go out first -- left alone the scheduler sank their reads below the
    // replica gathers, each behind its own lgkmcnt(0), four serial LDS round trips
    // per chunk; (2) every replica index; (3) every replica gather (the data
    // replica's first, at the prompt indices), then tap-major; (4) the rotated samples (the phasor
    // chain, under the gathers' latency); (5) the FMAs tap-major, so each tap's
    // FMAs wait only for that tap's gathers.  Every accumulator still adds its
    // samples in increasing j, so the sums are those of the sample-major order.
    const float cstep = q.cstep;
    const c2 ws = c2{q.wsx, q.wsy};
    c2 xs[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j)
        {
            const int n = n0 + (int)threadIdx.x + j * kTrkThreads;
            const int nc = FULL ? n : min(n, vl - 1);
            float2 v;
            if constexpr (SRC == 0)
                v = s_win[p.woff + nc];
            else if constexpr (SRC == 1)
                v = load_iq<IT>(iq, p.off + nc);
            else
                v = lds_iq<IT>(sbuf, sboff + nc * item_bytes<IT>());
            xs[j] = gsdr::pk::from(v);  // masked in phase 4: a select here waits for the load
        }
    __builtin_amdgcn_sched_barrier(0);
    float cv[SPL][KT];
    float dv[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j)
        {
            const int n0j = n0 + (int)threadIdx.x + j * kTrkThreads;
            const int n = FULL ? n0j : min(n0j, vl - 1);
            const float a = gsdr::mul_rn(cstep, (float)n);
#pragma unroll
            for (int k = 0; k < KT; ++k)
                {
                    // a_avx association: floor(step*n + (shift - rem))
                    int raw = floor_i(gsdr::add_rn(a, sh_rem[k]));
                    if (WRAP == 1)
                        {
                            raw += raw < 0 ? L : 0;
                            raw -= raw >= L ? L : 0;
                        }
                    else if (WRAP == 0)
                        raw = wrap_code(raw, L);
                    cv[j][k] = __int_as_float(raw);
                }
        }
    if (DATA && !PACK)
        {
            // first: the data replica is gathered at the prompt tap's index
#pragma unroll
            for (int j = 0; j < SPL; ++j) dv[j] = s_data[__float_as_int(cv[j][IPK])];
        }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        {
#pragma unroll
            for (int j = 0; j < SPL; ++j) cv[j][k] = s_code[__float_as_int(cv[j][k])];
        }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PACK)
        {
#pragma unroll
            for (int j = 0; j < SPL; ++j)
                {
                    if (DATA) dv[j] = half_hi(cv[j][IPK]);
#pragma unroll
                    for (int k = 0; k < KT; ++k) cv[j][k] = half_lo(cv[j][k]);
                }
        }
    c2 tt[SPL];
    c2 phv = gsdr::pk::from(ph);
#pragma unroll
    for (int j = 0; j < SPL; ++j)
        {
            if (!FULL && n0 + (int)threadIdx.x + j * kTrkThreads >= vl) xs[j] = c2{0.f, 0.f};
            tt[j] = gsdr::pk::mul(xs[j], phv);
            phv = gsdr::pk::mul(phv, ws);
        }
    ph = gsdr::pk::to(phv);
#pragma unroll
    for (int k = 0; k < KT; ++k)
        {
            c2 av = gsdr::pk::from(acc[k]);
#pragma unroll
            for (int j = 0; j < SPL; ++j) av = gsdr::pk::fmas(tt[j], cv[j][k], av);
            acc[k] = gsdr::pk::to(av);
        }
    if (DATA)
        {
            c2 av = gsdr::pk::from(acc[kMaxTrkTaps]);
#pragma unroll
            for (int j = 0; j < SPL; ++j) av = gsdr::pk::fmas(tt[j], dv[j], av);
            acc[kMaxTrkTaps] = gsdr::pk::to(av);
        }
}

// the chunk at n0 with the call's wrap mode; FULL when the whole chunk is inside the call
template <int IT, int SRC, int KT, bool DATA, int SPL, bool PACK>
__device__ __forceinline__ void correlate_chunk_wrap(const void* __restrict__ iq, const float2* s_win, const float* s_code,
    const float* s_data, const Prep& p, const ChunkNco& q, int n0, int vl, int L, const float (&sh_rem)[kMaxTrkTaps], float2& ph,
    float2 (&acc)[kMaxTrkTaps + 1], const char* sbuf, int sboff)
{
    if (q.wrap == 2)
        {
            if (SPL == kSpl && n0 + kWinCore <= vl)
                correlate_chunk<IT, SRC, 2, true, KT, DATA, SPL, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc,
                    sbuf, sboff);
            else
                correlate_chunk<IT, SRC, 2, false, KT, DATA, SPL, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc,
                    sbuf, sboff);
        }
    else if (q.wrap == 1)
        correlate_chunk<IT, SRC, 1, false, KT, DATA, SPL, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf,
            sboff);
    else
        correlate_chunk<IT, SRC, 0, false, KT, DATA, SPL, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf,
            sboff);
}

// A call's last chunk that holds fewer than kWinCore samples runs with as few
// samples per lane as cover it (1, 2, 4 or kSpl): a 25000-sample call's last 424
// samples take one sample per lane instead of a full chunk of masked ones.  The
// samples and their order are those of the full chunk (a masked sample adds 0).
template <int IT, int SRC, int KT, bool DATA, bool PACK = false>
__device__ __forceinline__ void correlate_chunk_any(const void* __restrict__ iq, const float2* s_win, const float* s_code,
    const float* s_data, const Prep& p, const ChunkNco& q, int n0, int vl, int L, const float (&sh_rem)[kMaxTrkTaps], float2& ph,
    float2 (&acc)[kMaxTrkTaps + 1], const char* sbuf = nullptr, int sboff = 0)
{
    const int rest = vl - n0;
    if (rest >= kWinCore || rest > 4 * kTrkThreads || kSpl <= 4)
        correlate_chunk_wrap<IT, SRC, KT, DATA, kSpl, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf, sboff);
    else if (rest > 2 * kTrkThreads)
        correlate_chunk_wrap<IT, SRC, KT, DATA, 4, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf, sboff);
    else if (rest > kTrkThreads)
        correlate_chunk_wrap<IT, SRC, KT, DATA, 2, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf, sboff);
    else
        correlate_chunk_wrap<IT, SRC, KT, DATA, 1, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc, sbuf, sboff);
}

// high_dyn correlation (do_correlation_step with set_high_dynamics_resampler(true)):
// VOLK-GNSSSDR 32f_xn_high_dynamics_resampler_32f_xn generic (:67-96: tap 0 index
// floor(step*m + rate*(m*m) + shift0 - rem) with the unsigned m*m, taps 1..K-1 the
// sample-shifted copies of tap 0) and 32fc_32f_high_dynamic_rotator_dot_prod_32fc_xn
// (:68-112: sample n rotated by the phase of n*theta + (n-1)^2*theta_rate, from the
// fp64 model as in corr.hip).  Lane-strided samples; the window or HBM as the fast path.
// (always inlined: as a call it took the address of the kernel's accumulators,
// which then lived in scratch for every correlation path)
template <int IT>
__device__ __forceinline__ void correlate_call_hd(const void* __restrict__ iq, const float2* s_win, const float* s_code,
    const float* s_data, const Prep& p, int vl, int L, int K, bool data, float shift0, float shiftP,
    float2 (&acc)[kMaxTrkTaps + 1])
{
    constexpr double kInvTwoPi = 0.15915494309189533576888376337251;
    auto index = [&](float shift, uint32_t m) {
        const float a = gsdr::mul_rn(p.code_step, (float)m);
        const float b = gsdr::mul_rn(p.code_rate, (float)(m * m));
        int raw = (int)floorf(gsdr::sub_rn(gsdr::add_rn(gsdr::add_rn(a, b), shift), p.rem_code));
        raw %= L;
        return raw < 0 ? raw + L : raw;
    };
    for (int n = (int)threadIdx.x; n < vl; n += kTrkThreads)
        {
            const float2 x = p.woff >= 0 ? s_win[p.woff + n] : load_iq<IT>(iq, p.off + n);
            double phi = p.psi0 + (double)n * p.theta;
            if (n > 0)
                {
                    const double m1 = (double)(n - 1);
                    phi += m1 * m1 * p.theta_rate;
                }
            const float ang = (float)fma(-rint(phi * kInvTwoPi), kTwoPi, phi);
            float sn, cs;
            sincosf(ang, &sn, &cs);
            const float2 tt = make_float2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
#pragma unroll
            for (int k = 0; k < kMaxTrkTaps; ++k)
                {
                    if (k < K)
                        {
                            const float cv = s_code[index(shift0, (uint32_t)((n + p.hdshift[k]) % vl))];
                            acc[k].x += tt.x * cv;
                            acc[k].y += tt.y * cv;
                        }
                }
            if (data)
                {
                    const float dv = s_data[index(shiftP, (uint32_t)n)];
                    acc[kMaxTrkTaps].x += tt.x * dv;
                    acc[kMaxTrkTaps].y += tt.y * dv;
                }
        }
}

template <int IT, int KT, bool DATA, bool PACK = false>
__device__ __forceinline__ void correlate_call(const void* __restrict__ iq, const float2* s_win, const float* s_code,
    const float* s_data, const Prep& p, int vl, int L, const float (&sh_rem)[kMaxTrkTaps], float2& ph,
    float2 (&acc)[kMaxTrkTaps + 1])
{
    const ChunkNco q = chunk_nco(p);
    for (int n0 = 0; n0 < vl; n0 += kWinCore)
        {
            if (p.woff >= 0)
                correlate_chunk_any<IT, 0, KT, DATA, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc);
            else
                correlate_chunk_any<IT, 1, KT, DATA, PACK>(iq, s_win, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc);
        }
}

// Streamed call (vector_length > kWinCore): the call's samples pass through two
// LDS chunk buffers of `chunk` samples filled by global_load_lds.  Chunk j is
// read from buffer j&1 while chunk j+1 lands in the other; chunk 0 was
// prefetched during the previous call's loop update when `pf_ok` (else fetched
// here).  The __syncthreads at the top of each chunk drains the DMA (vmcnt(0))
// and orders the previous chunk's reads before its buffer is refilled.
template <int IT, int KT, bool DATA, bool PACK = false>
__device__ __forceinline__ void correlate_call_stream(const void* __restrict__ iq, uint64_t iq_items, char* sb,
    int sbuf_bytes, int chunk, bool pf_ok, const uintptr_t (&pf_start)[2], const float* s_code, const float* s_data, const Prep& p,
    int vl, int L, const float (&sh_rem)[kMaxTrkTaps], float2& ph, float2 (&acc)[kMaxTrkTaps + 1], bool probe, uint64_t& swait)
{
    const ChunkNco q = chunk_nco(p);
    constexpr int isz = item_bytes<IT>();
    const uint64_t nbytes = iq_items * (uint64_t)isz;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(iq) + (uintptr_t)p.off * isz;  // byte address of sample 0
    uintptr_t bstart[2];
    if (!pf_ok)
        {
            // a prefetch into buffer 0 that missed this call may still be landing, its
            // rows from other waves than this fetch's: let it land before refilling
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    // a tail of at most kTrkThreads samples rides with the last whole chunk (the
    // buffers hold chunk + kTrkThreads items): no loop iteration of its own
    int nch = (vl + chunk - 1) / chunk;
    if (nch > 1 && vl - (nch - 1) * chunk <= kTrkThreads) --nch;
    auto len = [&](int j) { return j == nch - 1 ? vl - j * chunk : chunk; };
    bstart[0] = pf_ok ? pf_start[0] : stream_fetch(iq, nbytes, p.off * isz, len(0) * isz, sb, 0);
    bstart[1] = 0;
    // chunk 1 came with chunk 0 (into the other buffer) when the prefetch covered it
    const bool pf1 = pf_ok && pf_start[1] != 0 && nch > 1;
    if (pf1) bstart[1] = pf_start[1];
    for (int j = 0; j < nch; ++j)
        {
            // a workgroup barrier waits only on lgkmcnt and LDS DMA is tracked per
            // wave in vmcnt: every issuing wave drains its own DMA (chunk j, and for
            // j == 0 the prefetch waves 1.. issued during the previous loop update)
            // before the barrier hands the buffer to the other waves
            const uint64_t w0 = probe ? wall_clock64() : 0;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (probe) swait += wall_clock64() - w0;
            if (j + 1 < nch && !(j == 0 && pf1))
                bstart[(j + 1) & 1] =
                    stream_fetch(iq, nbytes, (p.off + (int64_t)(j + 1) * chunk) * isz, len(j + 1) * isz, sb + ((j + 1) & 1) * sbuf_bytes, 0);
            const char* buf = sb + (j & 1) * sbuf_bytes;
            const int boff = (int)((int64_t)s0 - (int64_t)bstart[j & 1]);
            const int nend = j * chunk + len(j);
            for (int n0 = j * chunk; n0 < nend;)
                {
                    // E/P/L calls: two kWinCore blocks as one chunk of 2 kSpl samples per lane
                    // where they are whole and need no wrap -- twice the gathers in flight per
                    // wait (the lane's samples and their order are those of the two blocks;
                    // five taps or the data tap at this width spill)
                    if (KT == 3 && !DATA && n0 + 2 * kWinCore <= nend && q.wrap == 2)
                        {
                            correlate_chunk<IT, 2, 2, true, KT, DATA, 2 * kSpl>(iq, nullptr, s_code, s_data, p, q, n0, vl, L,
                                sh_rem, ph, acc, buf, boff);
                            n0 += 2 * kWinCore;
                        }
                    else
                        {
                            correlate_chunk_any<IT, 2, KT, DATA, PACK>(iq, nullptr, s_code, s_data, p, q, n0, vl, L, sh_rem, ph, acc,
                                buf, boff);
                            n0 += kWinCore;
                        }
                }
        }
}

}  // namespace
