// Packed-f32 LDS Stockham FFT for CDNA4 (gfx950).
//
// Same transform and data flow as fft_lds.h / fft_multi.h (unnormalised forward
// DFT, first stage from a load functor, last stage to a store functor, S-1 LDS
// round trips), but every complex value lives in one 64-bit VGPR pair and every
// complex operation is issued as packed-f32 VALU (v_pk_add_f32 / v_pk_mul_f32 /
// v_pk_fma_f32 with op_sel / neg modifiers):
//
//   complex add/sub            1 instruction   (scalar f32: 2)
//   p +- (-i)q                 1 instruction   (scalar: 2, plus the swap)
//   complex * complex          2 instructions  (scalar: 4)
//   real * complex (+ complex) 1 instruction   (scalar: 2)
//
// A wave64 v_pk_* instruction issues in the same 4 cycles as a v_add_f32, so
// the butterflies cost about half the VALU issue slots of the scalar form --
// the acquisition correlate kernel is VALU-issue-bound.
//
// The swizzled forms the compiler does not fold into op_sel/neg modifiers are
// written as inline asm; tools/pk_semantics.hip checks their semantics on the
// device.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "fft_lds.h"
#include "fft_multi.h"

namespace gsdr
{
namespace pk
{

typedef float c2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ c2 from(float2 v) { return c2{v.x, v.y}; }
__device__ __forceinline__ float2 to(c2 v) { return make_float2(v.x, v.y); }

// a * b (complex)
__device__ __forceinline__ c2 mul(c2 a, c2 b)
{
    c2 r, o;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
        : "=v"(o)
        : "v"(a), "v"(b), "v"(r));
    return o;
}

// conj(a) * b
__device__ __forceinline__ c2 conj_mul(c2 a, c2 b)
{
    c2 r, o;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[1,0,0]"
        : "=v"(o)
        : "v"(a), "v"(b), "v"(r));
    return o;
}

// p + (-i) q = (p.x + q.y, p.y - q.x)
__device__ __forceinline__ c2 add_mi(c2 p, c2 q)
{
    c2 o;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(o) : "v"(p), "v"(q));
    return o;
}

// p - (-i) q = (p.x - q.y, p.y + q.x)
__device__ __forceinline__ c2 sub_mi(c2 p, c2 q)
{
    c2 o;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(o) : "v"(p), "v"(q));
    return o;
}

// (-i) a = (a.y, -a.x)
__device__ __forceinline__ c2 mul_mi(c2 a) { return a.yx * c2{1.0f, -1.0f}; }

// real scalar forms (the compiler emits one v_pk_mul / v_pk_fma with a broadcast operand)
__device__ __forceinline__ c2 scale(c2 a, float s) { return a * c2{s, s}; }
__device__ __forceinline__ c2 fmas(c2 a, float s, c2 c) { return __builtin_elementwise_fma(a, c2{s, s}, c); }

// a * w for a compile-time root w (special-cases 1, -1, +-i)
template <int M, int R>
__device__ __forceinline__ c2 mul_root(c2 a)
{
    constexpr int m = ((M % R) + R) % R;
    if constexpr (m == 0)
        return a;
    else if constexpr (4 * m == R)
        return mul_mi(a);
    else if constexpr (2 * m == R)
        return -a;
    else if constexpr (4 * m == 3 * R)
        return a.yx * c2{-1.0f, 1.0f};
    else
        {
            constexpr fft::Roots<R> W{};
            constexpr float wr = W.re[m], wi = W.im[m];
            // (a.x wr - a.y wi, a.y wr + a.x wi)
            const c2 t = a * c2{wr, wr};
            return __builtin_elementwise_fma(a.yx, c2{-wi, wi}, t);
        }
}

// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E-1
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F& f)
{
    if constexpr (B < E)
        {
            f(std::integral_constant<int, B>{});
            static_for<B + 1, E>(f);
        }
}

// ---- twiddle powers ----
// v[r] *= w1^r for r = 1 .. R-1 by one chain w <- w w1 (R-2 dependent complex
// products).  A baby-step / giant-step tree with a shorter dependency (r04e) was
// within noise at N = 4000 / 16000 / 32000 and 7 % slower on the 64000 split.
template <int R>
__device__ __forceinline__ void apply_powers(c2* v, c2 w1)
{
    c2 w = w1;
#pragma unroll
    for (int r = 1; r < R; ++r)
        {
            if (r > 1) w = mul(w, w1);
            v[r] = mul(v[r], w);
        }
}

// ---- small DFTs, natural order in and out, forward sign ----
template <int R>
struct Dft;

template <>
struct Dft<2>
{
    __device__ __forceinline__ static void run(c2* v)
    {
        const c2 a = v[0], b = v[1];
        v[0] = a + b;
        v[1] = a - b;
    }
};

template <>
struct Dft<3>
{
    __device__ __forceinline__ static void run(c2* v)
    {
        constexpr float h = 0.86602540378443864676f;  // sin(2pi/3)
        const c2 s = v[1] + v[2];
        const c2 d = v[1] - v[2];
        const c2 m = fmas(s, -0.5f, v[0]);
        const c2 t = scale(d, h);
        v[0] = v[0] + s;
        v[1] = add_mi(m, t);
        v[2] = sub_mi(m, t);
    }
};

template <>
struct Dft<4>
{
    __device__ __forceinline__ static void run(c2* v)
    {
        const c2 a = v[0] + v[2], b = v[0] - v[2];
        const c2 c = v[1] + v[3], d = v[1] - v[3];
        v[0] = a + c;
        v[2] = a - c;
        v[1] = add_mi(b, d);
        v[3] = sub_mi(b, d);
    }
};

template <>
struct Dft<5>
{
    __device__ __forceinline__ static void run(c2* v)
    {
        constexpr float c1 = 0.30901699437494742410f;   // cos(2pi/5)
        constexpr float c2_ = -0.80901699437494742410f;  // cos(4pi/5)
        constexpr float s1 = 0.95105651629515357212f;   // sin(2pi/5)
        constexpr float s2 = 0.58778525229247312917f;   // sin(4pi/5)
        const c2 a1 = v[1] + v[4], b1 = v[1] - v[4];
        const c2 a2 = v[2] + v[3], b2 = v[2] - v[3];
        const c2 x0 = v[0];
        const c2 p1 = fmas(a2, c2_, fmas(a1, c1, x0));
        const c2 p2 = fmas(a2, c1, fmas(a1, c2_, x0));
        const c2 q1 = fmas(b2, s2, scale(b1, s1));
        const c2 q2 = fmas(b2, -s1, scale(b1, s2));
        v[0] = x0 + a1 + a2;
        v[1] = add_mi(p1, q1);
        v[4] = sub_mi(p1, q1);
        v[2] = add_mi(p2, q2);
        v[3] = sub_mi(p2, q2);
    }
};

// The 5-point DFT in 16 packed instructions instead of Dft<5>'s 18: with s = a1 + a2 and
// d = a1 - a2, cos(2pi/5) a1 + cos(4pi/5) a2 = -s/4 + (sqrt(5)/4) d (and the two swapped:
// - (sqrt(5)/4) d), and sin(2pi/5) = s1 is taken out of q1 = s1 (b1 + (s2/s1) b2) and
// q2 = s1 ((s2/s1) b1 - b2), to ride in the fused multiply-add that forms an output
// p +- (-i) s1 t.  Other roundings than Dft<5>'s (f32 against f64 on 200,000 random inputs:
// rms error 1.84e-7 against 1.70e-7, largest 1.38e-6 against 1.28e-6), so it is a transform
// of its own for plans that choose it (PkPfaPlan4000Lean), not a form of Dft<5>.
template <int R>
struct DftLean;

template <>
struct DftLean<5>
{
    static constexpr float s1 = 0.95105651629515357212f;  // sin(2pi/5)
    // output 0 and the halves of the pairs: outputs 1, 4 = p1 +- (-i) s1 t1, outputs 2, 3 = p2 +- (-i) s1 t2
    struct Halves
    {
        c2 y0, p1, p2, t1, t2;
    };
    __device__ __forceinline__ static Halves halves(const c2* v)
    {
        constexpr float r = 0.55901699437494742410f;   // sqrt(5) / 4
        constexpr float k = 0.61803398874989484820f;   // sin(4pi/5) / sin(2pi/5)
        const c2 a1 = v[1] + v[4], b1 = v[1] - v[4];
        const c2 a2 = v[2] + v[3], b2 = v[2] - v[3];
        const c2 x0 = v[0];
        const c2 s = a1 + a2, d = a1 - a2;
        const c2 m = fmas(s, -0.25f, x0);
        Halves h;
        h.y0 = x0 + s;
        h.p1 = fmas(d, r, m);
        h.p2 = fmas(d, -r, m);
        h.t1 = fmas(b2, k, b1);
        h.t2 = fmas(b1, k, -b2);
        return h;
    }
    // p + (-i) s1 t = (p.x + s1 t.y, p.y - s1 t.x) and p - (-i) s1 t
    __device__ __forceinline__ static c2 plus(c2 p, c2 t) { return __builtin_elementwise_fma(t.yx, c2{s1, -s1}, p); }
    __device__ __forceinline__ static c2 minus(c2 p, c2 t) { return __builtin_elementwise_fma(t.yx, c2{-s1, s1}, p); }
    // the same two points as their real parts (p.x + s1 t.y, p.x - s1 t.y) and their imaginary
    // parts (p.y - s1 t.x, p.y + s1 t.x), for a consumer that works on both points at once
    __device__ __forceinline__ static c2 pair_re(c2 p, c2 t) { return __builtin_elementwise_fma(t.yy, c2{s1, -s1}, p.xx); }
    __device__ __forceinline__ static c2 pair_im(c2 p, c2 t) { return __builtin_elementwise_fma(t.xx, c2{-s1, s1}, p.yy); }
    __device__ __forceinline__ static void run(c2* v)
    {
        const Halves h = halves(v);
        v[0] = h.y0;
        v[1] = plus(h.p1, h.t1);
        v[4] = minus(h.p1, h.t1);
        v[2] = plus(h.p2, h.t2);
        v[3] = minus(h.p2, h.t2);
    }
};

// Composite R = R1*R2 in registers: n = R2*n1 + n2, k = k1 + R1*k2, on the small transforms
// D<R1> and D<R2> (Dft, or DftLean for DftCT<5, 5, DftLean>).
template <int R1, int R2, template <int> class D = Dft>
struct DftCT
{
    template <int N2, int K1>
    __device__ __forceinline__ static void twiddle(c2* t)
    {
        t[K1] = mul_root<N2 * K1, R1 * R2>(t[K1]);
        if constexpr (K1 + 1 < R1) twiddle<N2, K1 + 1>(t);
    }
    template <int N2>
    __device__ __forceinline__ static void cols(c2* v, c2* y)
    {
        c2 t[R1];
#pragma unroll
        for (int n1 = 0; n1 < R1; ++n1) t[n1] = v[R2 * n1 + N2];
        D<R1>::run(t);
        twiddle<N2, 0>(t);
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1) y[N2 * R1 + k1] = t[k1];
        if constexpr (N2 + 1 < R2) cols<N2 + 1>(v, y);
    }
    __device__ __forceinline__ static void run(c2* v)
    {
        c2 y[R1 * R2];
        cols<0>(v, y);
#pragma unroll
        for (int k1 = 0; k1 < R1; ++k1)
            {
                c2 t[R2];
#pragma unroll
                for (int n2 = 0; n2 < R2; ++n2) t[n2] = y[n2 * R1 + k1];
                D<R2>::run(t);
#pragma unroll
                for (int k2 = 0; k2 < R2; ++k2) v[k1 + R1 * k2] = t[k2];
            }
    }
};

template <>
struct Dft<6> : DftCT<2, 3>
{
};
template <>
struct Dft<8> : DftCT<2, 4>
{
};
template <>
struct Dft<10> : DftCT<2, 5>
{
};
template <>
struct Dft<12> : DftCT<4, 3>
{
};
template <>
struct Dft<16> : DftCT<4, 4>
{
};
template <>
struct Dft<20> : DftCT<4, 5>
{
};
template <>
struct Dft<25> : DftCT<5, 5>
{
};
template <>
struct Dft<32> : DftCT<4, 8>
{
};

// One Stockham stage over an N-point LDS buffer of c2.
//   TWP: inter-stage twiddles as powers of one table root (1 VMEM load per
//        butterfly, R-2 extra complex multiplies); else R-1 table loads.
//   ORD: the last stage hands each lane its outputs in increasing index order (a
//        first-maximum scan needs it); without ORD it visits butterfly by
//        butterfly, so a partially filled pass is skipped as a whole instead of
//        predicating every output (order-free reductions: max, sum).
// Measured and removed: twiddles from a per-stage table (-23 %)
// or an LDS copy of the middle stage's roots (-2.5 %), last-stage block padding
// (modelled conflicts removed, no gain), the barrier moved behind the butterflies
// or dropped before the last stage (within noise).
//
// Two more caller hooks, both NoHook unless PkPlan::run is given them:
//   pre(): before the first stage's LDS writes, after its butterflies, outside
//          any per-lane guard (a caller that kept operands in the buffer puts its
//          barrier here);
//   mid(): in the last stage between its barrier and its butterflies -- every
//          lane's inputs are in registers, the buffer is dead until the next
//          transform's first stage writes it.
struct NoHook
{
    __device__ __forceinline__ void operator()() const {}
};

// Where the inter-stage twiddles come from.  TwGlobal: the table `tw` in global
// memory, as TWP says (every caller's default).  Any other type is a caller's own
// source of the same values (TWP plans only), e.g. tables in its LDS, read beside
// the stage's inputs, ahead of its barrier:
//   Mid<R>                  what a middle stage of radix R holds per butterfly;
//   load_middle<R, Ns>(k)   -> Mid<R> for w = tw[k N / (Ns R)] -- a stage that is
//                           neither the first nor the last;
//   middle<R>(v, m)         v[r] *= w^r for r = 1 .. R-1, with the bits of
//                           apply_powers' chain;
//   last_root(k)            tw[k], the last stage's root; apply_powers runs on it.
// Such a source needs no early global load ahead of the last stage's barrier (MID
// below).
struct TwGlobal
{
    template <int R>
    using Mid = c2;
};

template <int R, int NT, int N, int Ns, bool TWP, bool FIRST, bool LAST, bool ORD, bool SKIPW, class Load, class Store,
    class Hook, class Pre, class Mid, class Tws>
__device__ __forceinline__ void stage(c2* lds, const float2* __restrict__ tw, Load& load, Store& store, Hook& hook,
    Pre& pre, Mid& mid, const Tws& tws)
{
    constexpr bool GLOBAL = std::is_same<Tws, TwGlobal>::value;
    static_assert(GLOBAL || TWP, "a twiddle source stands for the roots of a TWP plan");
    constexpr int BPT = fft::bpt_for(R);
    // with a pre() hook the first stage's writes follow every pass's butterflies
    constexpr bool PRE = FIRST && !LAST && !std::is_same<Pre, NoHook>::value;
    // with a mid() hook the last stage's twiddle roots are loaded ahead of its
    // barrier: a load issued after the hook's would wait for them too (vmcnt counts
    // in order)
    constexpr bool MID = LAST && !FIRST && TWP && GLOBAL && !std::is_same<Mid, NoHook>::value;
    constexpr int NB = N / R;
    constexpr int TSTRIDE = N / (Ns * R);
    c2 v[BPT][R];
    c2 w1[BPT];
    std::conditional_t<LAST, c2, typename Tws::template Mid<R>> tf[BPT];
    if constexpr (MID)
        {
            // (every lane, the idle ones from a clamped index: no branch)
#pragma unroll
            for (int b = 0; b < BPT; ++b) w1[b] = from(tw[(min(threadIdx.x + (unsigned)(b * NT), (unsigned)(NB - 1)) % Ns) * TSTRIDE]);
        }
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            // one pass per lane (BPT == 1): every lane loads, the idle ones from a
            // clamped in-bounds index -- no branch around the loads, so no
            // zero-filled registers for the idle lanes; their results are never
            // stored.  Several passes: the per-lane guard.
            const int j = (int)threadIdx.x + b * NT;
            if constexpr (BPT == 1 && NB % NT != 0)
                {
                    const int jj = min(j, NB - 1);
                    // SKIPW: a wave without any butterfly of the first stage skips its loads
                    // (and whatever the load functor computes) on a wave-uniform branch
                    if (!FIRST || !SKIPW || __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) < NB)
                        {
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                {
                                    if constexpr (FIRST)
                                        v[b][r] = load(b, r, jj + r * NB);
                                    else
                                        v[b][r] = lds[jj + r * NB];
                                }
                        }
                }
            else if (NB % NT == 0 || j < NB)
                {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        {
                            if constexpr (FIRST)
                                v[b][r] = load(b, r, j + r * NB);
                            else
                                v[b][r] = lds[j + r * NB];
                        }
                }
        }
    if constexpr (FIRST)
        hook();
    else
        {
            if constexpr (!GLOBAL)
                {
                    // (every lane, the idle ones from a clamped index)
#pragma unroll
                    for (int b = 0; b < BPT; ++b)
                        {
                            const int k = min((int)threadIdx.x + b * NT, NB - 1) % Ns;
                            if constexpr (LAST)
                                tf[b] = tws.last_root(k * TSTRIDE);
                            else
                                tf[b] = tws.template load_middle<R, Ns>(k);
                        }
                }
            if constexpr (MID)
                {
                    // the roots have arrived before the barrier, so before mid()
#pragma unroll
                    for (int b = 0; b < BPT; ++b) asm volatile("" : "+v"(w1[b]));
                }
            __syncthreads();
            if constexpr (LAST) mid();
        }
#pragma unroll
    for (int b = 0; b < BPT; ++b)
        {
            const int j = (int)threadIdx.x + b * NT;
            if (NB % NT == 0 || j < NB)
                {
                    int k = 0;
                    if constexpr (!FIRST)
                        {
                            k = j % Ns;
                            const int step = k * TSTRIDE;
                            if constexpr (!GLOBAL)
                                {
                                    if constexpr (LAST)
                                        apply_powers<R>(v[b], tf[b]);
                                    else
                                        tws.template middle<R>(v[b], tf[b]);
                                }
                            else if constexpr (MID)
                                apply_powers<R>(v[b], w1[b]);
                            else if constexpr (TWP)
                                apply_powers<R>(v[b], from(tw[step]));
                            else
                                {
#pragma unroll
                                    for (int r = 1; r < R; ++r) v[b][r] = mul(v[b][r], from(tw[r * step]));
                                }
                        }
                    Dft<R>::run(v[b]);
                    if constexpr (!LAST && !PRE)
                        {
                            // block (j - k) R / (Ns R) = j / Ns of the last stage's input
                            const int base = (j - k) * R + k;
#pragma unroll
                            for (int r = 0; r < R; ++r) lds[base + r * Ns] = v[b][r];
                        }
                }
        }
    if constexpr (PRE)
        {
            pre();
#pragma unroll
            for (int b = 0; b < BPT; ++b)
                {
                    const int j = (int)threadIdx.x + b * NT;
                    if (NB % NT == 0 || j < NB)
                        {
                            // first stage: Ns = 1, k = 0
#pragma unroll
                            for (int r = 0; r < R; ++r) lds[j * R + r * Ns] = v[b][r];
                        }
                }
        }
    if constexpr (LAST && ORD)
        {
            // last stage: Ns = N/R and k = j, so output j + r*Ns; r outer, b inner
            // visits this lane's outputs in increasing index order, and the
            // compile-time slot r*BPT + b numbers them in that order
            static_assert(!LAST || Ns * R == N, "last stage");
#pragma unroll
            for (int r = 0; r < R; ++r)
                {
#pragma unroll
                    for (int b = 0; b < BPT; ++b)
                        {
                            const int j = (int)threadIdx.x + b * NT;
                            if (NB % NT == 0 || j < NB) store(j + r * Ns, v[b][r], r * BPT + b);
                        }
                }
        }
    else if constexpr (LAST)
        {
            static_assert(!LAST || Ns * R == N, "last stage");
#pragma unroll
            for (int b = 0; b < BPT; ++b)
                {
                    const int j = (int)threadIdx.x + b * NT;
                    if (NB % NT == 0 || j < NB)
                        {
#pragma unroll
                            for (int r = 0; r < R; ++r) store(j + r * Ns, v[b][r], r * BPT + b);
                        }
                }
        }
    else
        __syncthreads();
}

template <int NT, int N, int Ns, bool TWP, bool FIRST, bool ORD, bool SKIPW, int R, int... Rest, class Load, class Store,
    class Hook, class Pre, class Mid, class Tws>
__device__ __forceinline__ void stages(c2* lds, const float2* __restrict__ tw, Load& load, Store& store, Hook& hook,
    Pre& pre, Mid& mid, const Tws& tws)
{
    constexpr bool LAST = sizeof...(Rest) == 0;
    stage<R, NT, N, Ns, TWP, FIRST, LAST, ORD, SKIPW>(lds, tw, load, store, hook, pre, mid, tws);
    if constexpr (!LAST) stages<NT, N, Ns * R, TWP, false, ORD, SKIPW, Rest...>(lds, tw, load, store, hook, pre, mid, tws);
}

// Compile-time packed plan.  load(b, r, i) -> c2 returns input element i
// (= j + r*N/R1 of this lane's b-th first-stage butterfly j); store(i, c2)
// consumes output element i, visited in increasing i per lane; hook() runs
// once the first stage's inputs are in registers (before its butterflies);
// pre() and mid() are stage()'s optional hooks, SKIPW its switch for a first stage
// that leaves whole waves without a butterfly, tws its twiddle source (TwGlobal: tw).
//   TWP: inter-stage twiddles as powers of one loaded root (1) or R-1 loads (0).
template <int NT_, int TWP_, int... Rs>
struct PkPlan
{
    static constexpr int NT = NT_;
    static constexpr bool TWP = TWP_ != 0;
    static constexpr int N = (Rs * ...);
    static constexpr int nstages = sizeof...(Rs);
    static constexpr bool PRIME_FACTOR = false;  // (PkPfaPlan4000 below: first-stage inputs by its own index map)
    static constexpr bool PAIRS = false;         // (and its forms that hand the store functor two outputs at a time)
    static constexpr int R1 = fft::FirstRadix<Rs...>::value;
    static constexpr int BPT1 = fft::bpt_for(R1);
    static constexpr int NB1 = N / R1;
    static constexpr size_t lds_bytes() { return (size_t)N * sizeof(c2); }
    // last stage: radix, butterflies per thread, output stride; store(i, v, slot)
    // receives slot = r*BPTL + b in [0, RL*BPTL), this lane's output order
    static constexpr int RL = (0, ..., Rs);
    static constexpr int BPTL = fft::bpt_for(RL);
    static constexpr int NSL = N / RL;
    static constexpr int NSLOTS = RL * BPTL;
    __device__ __forceinline__ static int index_of_slot(int slot)
    {
        return (int)threadIdx.x + (slot % BPTL) * NT + (slot / BPTL) * NSL;
    }
    template <bool ORD = true, bool SKIPW = false, class Load, class Store, class Hook, class Pre = NoHook, class Mid = NoHook,
        class Tws = TwGlobal>
    __device__ __forceinline__ static void run(c2* lds, const float2* __restrict__ tw, Load load, Store store, Hook hook,
        Pre pre = Pre{}, Mid mid = Mid{}, Tws tws = Tws{})
    {
        stages<NT, N, 1, TWP, true, ORD, SKIPW, Rs...>(lds, tw, load, store, hook, pre, mid, tws);
    }
};

// ---- prime-factor plan, N = 4000 = 32 x 125 ----
// gcd(32, 125) = 1, so by Good-Thomas the 4000-point DFT is a true 32 x 125 two-
// dimensional DFT, no twiddle between the dimensions: with i = (125 n1 + 32 n2) mod N and
// k = (2625 k1 + 1376 k2) mod N, W_N^(i k) = W_32^(n1 k1) W_125^(n2 k2).  The stages keep
// PkPlan<256,1,25,16,10>'s radices, read as 125 = 25 x 5 (n2 = 5 m + c, k2 = k25 + 25 k5)
// and 32 = 16 x 2 (n1 = 2 m' + e, k1 = k16 + 16 k2'):
//   A  radix 25 over m, 160 butterflies, lane t = 5 n1 + c; output k25 to slot
//      25 t + k25 = 125 n1 + 25 c + k25 (first_index / first_slot: the lane-order image);
//   B  radix 16 over m', 250 butterflies, no twiddles: lane j = 125 e + 25 c + k25 reads
//      slots j + 250 m' and writes output k16 to j + 250 k16 -- the slots it alone read, and
//      a wave's LDS operations execute in order, so no barrier between reads and writes;
//   C  400 butterflies of 2 x 5 points in two passes, lane numbering k16 fastest (k16 =
//      j mod 16, k25 = j div 16: both passes of a lane share k16, and the 32 lanes of a
//      ds_read_b64 group touch 32 different slots mod 32); input (e, c) at slot
//      250 k16 + k25 + 125 e + 25 c.  u[1][c] *= W_32^k16 (one root), Dft<2> over e, both
//      halves times W_125^(c k25), c = 1 .. 4, Dft<5> over c: a prime-factor butterfly, no
//      internal W_10 twiddles.  Output (k2', k5) is frequency output_index().
// Against the 25 x 16 x 10 Stockham plan: no middle-stage twiddles, 13 twiddle products in
// a last-stage butterfly instead of 17 + the 4 of DftCT<2,5>, one barrier fewer.  The
// outputs come in an order of their own, for order-free statistics (ORD = false) only.
// run() has PkPlan::run's interface; load(0, r, i) gets the natural index
// i = first_index(j, r), and tws is a source of the two root tables:
//   tws.root32(k)            W_32^k, k < 16
//   tws.root125(k)           W_125^k, k < 25; the stage forms W_125^(c k), c = 2 .. 4, by a
//                            three-product chain (the powers read from a table instead:
//                            measured, -2 %, profiles/pfa101)
// both read beside the last stage's inputs, ahead of its barrier.
//
// LEAN: the butterflies on DftLean<5> -- the first stage DftCT<5, 5, DftLean>, and the last
// stage hands the store functor outputs 1, 4 and 2, 3 of each 5-point transform two at a time,
// store.pair(re, im) with the two points' real parts and imaginary parts, each one fused
// multiply-add from p and t (DftLean<5>::pair_re / pair_im), for a statistic that can work on
// two points in one packed instruction; output 0 takes store(i, v, slot).  A pair comes without
// an index: order-free statistics that ignore it only.  Other roundings than Dft<5>'s.
template <int NT_, bool LEAN>
struct PkPfaPlan4000Form
{
    static constexpr bool PAIRS = LEAN;  // the store functor has pair(re, im)
    static_assert(NT_ == 256, "160 / 250 / 2 x 200 butterflies on 256 lanes");
    static constexpr int NT = NT_;
    static constexpr bool TWP = true;
    static constexpr int N = 4000;
    static constexpr int nstages = 3;
    static constexpr bool PRIME_FACTOR = true;
    static constexpr int R1 = 25, BPT1 = 1, NB1 = 160;
    static constexpr int R2 = 16, NB2 = 250;
    static constexpr int RL = 10, BPTL = 2, NSL = 400, NSLOTS = RL * BPTL;
    static constexpr size_t lds_bytes() { return (size_t)N * sizeof(c2); }
    // stage A: natural index of input m of lane j = 5 n1 + c, and the slot of its output k25
    static constexpr int first_index(int j, int m) { return (125 * (j / 5) + 32 * (j % 5) + 160 * m) % N; }
    static constexpr int first_slot(int j, int k25) { return 25 * j + k25; }
    // stage B: slot of input m' and of output k16 of lane j
    static constexpr int middle_slot(int j, int r) { return j + NB2 * r; }
    // stage C: slot of input (e, c) of butterfly (k16, k25); frequency of its output (k2', k5)
    static constexpr int last_slot(int k16, int k25, int e, int c) { return 250 * k16 + k25 + 125 * e + 25 * c; }
    static constexpr int output_index(int k16, int k25, int k2, int k5)
    {
        return (2625 * (k16 + 16 * k2) + 1376 * (k25 + 25 * k5)) % N;
    }

    template <bool ORD = false, bool SKIPW = false, class Load, class Store, class Hook, class Pre, class Mid, class Tws>
    __device__ __forceinline__ static void run(c2* lds, const float2* __restrict__, Load load, Store store, Hook hook, Pre,
        Mid mid, Tws tws)
    {
        static_assert(!ORD, "the outputs are not visited in index order");
        static_assert(std::is_same<Pre, NoHook>::value, "no pre() hook: the first stage takes the ordinary write path");
        const int t = (int)threadIdx.x;
        // ---- A
        {
            c2 v[R1];
            const int jj = min(t, NB1 - 1);
            // SKIPW: as stage() -- a wave without a butterfly skips the loads
            if (!SKIPW || __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) < NB1)
                {
#pragma unroll
                    for (int r = 0; r < R1; ++r) v[r] = load(0, r, first_index(jj, r));
                }
            hook();
            if (t < NB1)
                {
                    if constexpr (LEAN)
                        DftCT<5, 5, DftLean>::run(v);
                    else
                        Dft<R1>::run(v);
#pragma unroll
                    for (int r = 0; r < R1; ++r) lds[first_slot(t, r)] = v[r];
                }
            __syncthreads();
        }
        // ---- B (in place; the idle lanes read a clamped index and write nothing)
        {
            c2 v[R2];
            const int jj = min(t, NB2 - 1);
#pragma unroll
            for (int r = 0; r < R2; ++r) v[r] = lds[middle_slot(jj, r)];
            if (t < NB2)
                {
                    Dft<R2>::run(v);
#pragma unroll
                    for (int r = 0; r < R2; ++r) lds[middle_slot(t, r)] = v[r];
                }
            __syncthreads();
        }
        // ---- C
        {
            c2 v[BPTL][RL];
            c2 w125[BPTL][4];
            const int k16 = t & 15, k25 = t >> 4;      // second pass: k25 + 16, lanes below 144
            const int k25b = min(k25 + 16, 24);
            const c2 w32 = tws.root32(k16);
            w125[0][0] = tws.root125(k25);
            w125[1][0] = tws.root125(k25b);
            // The inputs as single ds_read_b64 (banked mod 64: conflict-free in this numbering; the
            // ds_read2_b64 pairs the compiler would form are banked mod 32, two-way conflicts).  The
            // compiler does not count these reads, so the stage waits for them itself, as TwLds::middle
            // does: the second pass's wait stands in the statement of its reads, the first pass's
            // registers are named behind the wait, ahead of their first use.
            const unsigned a0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(lds + last_slot(k16, k25, 0, 0));
            const unsigned a1 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(lds + last_slot(k16, k25b, 0, 0));
            static_assert(last_slot(0, 0, 0, 1) * 8 == 200 && last_slot(0, 0, 1, 0) * 8 == 1000, "the offsets below");
#define GSDR_PFA_READS                                                                                           \
    "ds_read_b64 %0, %10\n\tds_read_b64 %1, %10 offset:200\n\tds_read_b64 %2, %10 offset:400\n\t"              \
    "ds_read_b64 %3, %10 offset:600\n\tds_read_b64 %4, %10 offset:800\n\tds_read_b64 %5, %10 offset:1000\n\t"  \
    "ds_read_b64 %6, %10 offset:1200\n\tds_read_b64 %7, %10 offset:1400\n\tds_read_b64 %8, %10 offset:1600\n\t" \
    "ds_read_b64 %9, %10 offset:1800"
#define GSDR_PFA_REGS(B)                                                                                         \
    "=&v"(v[B][0]), "=&v"(v[B][1]), "=&v"(v[B][2]), "=&v"(v[B][3]), "=&v"(v[B][4]), "=&v"(v[B][5]), "=&v"(v[B][6]),  \
        "=&v"(v[B][7]), "=&v"(v[B][8]), "=&v"(v[B][9])
            asm volatile(GSDR_PFA_READS : GSDR_PFA_REGS(0) : "v"(a0) : "memory");
            // (a wave without a butterfly in the second pass skips its reads)
            if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) < NSL - NT)
                asm volatile(GSDR_PFA_READS "\n\ts_waitcnt lgkmcnt(0)" : GSDR_PFA_REGS(1) : "v"(a1) : "memory");
            else
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#undef GSDR_PFA_READS
#undef GSDR_PFA_REGS
#pragma unroll
            for (int r = 0; r < RL; ++r) asm volatile("" : "+v"(v[0][r]));
            __syncthreads();
            // every lane's inputs are in registers: the buffer is dead until the next first stage
            mid();
#pragma unroll
            for (int b = 0; b < BPTL; ++b)
                {
                    if (b == 0 || t < NSL - NT)
                        {
                            c2* u = v[b];  // u[5 e + c]
#pragma unroll
                            for (int c = 0; c < 5; ++c) u[5 + c] = mul(u[5 + c], w32);
#pragma unroll
                            for (int c = 0; c < 5; ++c)
                                {
                                    const c2 p = u[c], q = u[5 + c];
                                    u[c] = p + q;
                                    u[5 + c] = p - q;
                                }
                            c2* w = w125[b];
                            w[1] = mul(w[0], w[0]);
                            w[2] = mul(w[1], w[0]);
                            w[3] = mul(w[2], w[0]);
#pragma unroll
                            for (int c = 1; c < 5; ++c)
                                {
                                    u[c] = mul(u[c], w[c - 1]);
                                    u[5 + c] = mul(u[5 + c], w[c - 1]);
                                }
                            const int kk = k25 + 16 * b;
                            if constexpr (LEAN)
                                {
#pragma unroll
                                    for (int e = 0; e < 2; ++e)
                                        {
                                            const auto h = DftLean<5>::halves(u + 5 * e);
                                            store(output_index(k16, kk, e, 0), h.y0, 5 * e * BPTL + b);
                                            store.pair(DftLean<5>::pair_re(h.p1, h.t1), DftLean<5>::pair_im(h.p1, h.t1));
                                            store.pair(DftLean<5>::pair_re(h.p2, h.t2), DftLean<5>::pair_im(h.p2, h.t2));
                                        }
                                }
                            else
                                {
                                    Dft<5>::run(u);
                                    Dft<5>::run(u + 5);
#pragma unroll
                                    for (int r = 0; r < RL; ++r) store(output_index(k16, kk, r / 5, r % 5), u[r], r * BPTL + b);
                                }
                        }
                }
        }
    }
};

template <int NT_>
struct PkPfaPlan4000 : PkPfaPlan4000Form<NT_, false>
{
};
template <int NT_>
struct PkPfaPlan4000Lean : PkPfaPlan4000Form<NT_, true>
{
};

// A last-stage store functor of two: one(i, v, slot) for single outputs, two(re, im) for
// the pairs of a plan with PAIRS.
template <class One, class Two>
struct PairStore
{
    One one;
    Two two;
    __device__ __forceinline__ void operator()(int i, c2 v, int slot) { one(i, v, slot); }
    __device__ __forceinline__ void pair(c2 re, c2 im) { two(re, im); }
};

}  // namespace pk
}  // namespace gsdr
