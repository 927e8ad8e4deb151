// Tracking: the Kalman loop's filter step (wave 1), its LDS and its hand-off to wave 0.
#pragma once
#include "trk_loop.h"

// The reference loop is compiled for x86-64 without FMA contraction; keep every
// a*b+c of the restatement as two roundings.
#pragma clang fp contract(off)

namespace
{
using namespace gsdr::trk;

// ------------------------------------------------------------------ Kalman loop
// run_Kf (kf_tracking.cc:1129-1204) on wave 1, the covariance algebra spread over its
// lanes: lane l (mod 16) owns element (i, j) = (l / 4, l % 4) of every 4x4 matrix, the
// 4x2 and 2x2 ones sit on the lanes with j < 2 (and i < 2); a product's other operands
// come through cross-lane reads.  d_F = I + five entries above the diagonal and d_H =
// [I2 | four entries], so each product is the lane's own element and two terms (kf_model
// holds the nine entries); FP64 as the reference's arma::mat; the 2x2 inverse in closed
// form.  x (4 values) is uniform across the lanes.
struct KfModel
{
    double f02, f03, f12, f13, f23;  // d_F (init_kf, :863-866)
    double h02, h03, h12, h13;       // d_H (:868-869)
};

__host__ __device__ inline KfModel kf_model(double beta, double Ti)
{
    const double TiTi = Ti * Ti;
    return KfModel{beta * Ti, beta * TiTi / 2.0, 2.0 * kGnssPi * Ti, kGnssPi * TiTi, Ti, -beta * Ti / 2.0, beta * TiTi / 6.0,
        -kGnssPi * Ti, kGnssPi * TiTi / 3.0};
}

// d_R from a C/N0 (update_kf_cn0, :947-954; update_kf_narrow_integration_time, :921-927)
__host__ __device__ inline void kf_r_of_cn0(double cn0_db_hz, double Ti, float spc_f, double (&R)[2])
{
    const double spc = (double)spc_f;
    const double CN0_lin = pow(10.0, cn0_db_hz / 10.0);
    const double CN0_lin_Ti = CN0_lin * Ti;
    const double Sigma2_Phase = (1.0 / (2.0 * CN0_lin_Ti)) * (1.0 + 1.0 / (2.0 * CN0_lin_Ti));
    const double Sigma2_Tau = (1.0 / CN0_lin_Ti) * (spc + (spc / (1.0 - spc)) * (1.0 / (2.0 * CN0_lin_Ti)));
    R[0] = Sigma2_Tau;
    R[1] = Sigma2_Phase;
}

__device__ __forceinline__ double lane_d(double v, int i)  // i uniform
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), i);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// element (i, j) of F X F^T from the lane's element x of X: A = F X takes rows 2 and 3 of
// X in the lane's column, A F^T columns 2 and 3 of A in the lane's row
__device__ __forceinline__ double kf_fxft(const KfModel& m, double x, int i, int j)
{
    const double fi2 = i == 0 ? m.f02 : (i == 1 ? m.f12 : 0.0);
    const double fi3 = i == 0 ? m.f03 : (i == 1 ? m.f13 : (i == 2 ? m.f23 : 0.0));
    const double fj2 = j == 0 ? m.f02 : (j == 1 ? m.f12 : 0.0);
    const double fj3 = j == 0 ? m.f03 : (j == 1 ? m.f13 : (j == 2 ? m.f23 : 0.0));
    const double a = x + fi2 * __shfl(x, 8 + j) + fi3 * __shfl(x, 12 + j);
    return a + fj2 * __shfl(a, 4 * i + 2) + fj3 * __shfl(a, 4 * i + 3);
}

// The discriminators of run_Kf (:1131-1151) with their float library calls correctly
// rounded (see cn0_and_lock): pll_cloop_two_quadrant_atan / pll_four_quadrant_atan and
// dll_nc_e_minus_l_normalized; dll_nc_vemlp calls none
[[maybe_unused]] __device__ inline double kf_carrier_disc(int cloop, float2 p)
{
    if (!cloop) return (double)(float)atan2((double)p.y, (double)p.x);
    if (p.x != 0.0F) return (double)(float)atan((double)(p.y / p.x));
    return 0.0;
}

[[maybe_unused]] __device__ inline double kf_dll_nc_e_minus_l(float2 e, float2 l, float spc, float slope, float y)
{
    // the products of floats are exact in double: one rounding in the sum, one in the root
    const double pe = (double)(float)sqrt((double)e.x * (double)e.x + (double)e.y * (double)e.y);
    const double pl = (double)(float)sqrt((double)l.x * (double)l.x + (double)l.y * (double)l.y);
    const double s = pe + pl;
    if (s == 0.0) return 0.0;
    return (double)((y - slope * spc) / slope) * (pe - pl) / s;
}

struct KfSlot  // x and P of a channel: the current one and the one wave 1 steps into
{
    double x[4], P[16];
};

struct KfPred
{
    double xm[4];  // d_x_new_old
    double Pm;     // d_P_new_old(i, j)
    double M;      // (d_P_new_old * d_H.t())(i, j), lanes with j < 2
    double HP;     // (d_H * d_P_new_old)(i, j), lanes with i < 2
};

// Prediction, P- H^T and H P- (:1156-1158 and the first products of :1162): nothing here
// depends on the call's lock test.  Every product sums its terms in ascending index with two
// roundings per term, as Armadillo's fixed-size 4x4 code does without FMA (the terms F and H
// make zero change nothing), so the step is the restatement's bit for bit.
[[maybe_unused]] __device__ __forceinline__ KfPred kf_predict(const KfModel& m, const KfSlot& s, const double* Q, int lane)
{
    const int l = lane & 15, i = l >> 2, j = l & 3;
    KfPred r;
    const double x0 = s.x[0], x1 = s.x[1], x2 = s.x[2], x3 = s.x[3];
    r.xm[0] = x0 + m.f02 * x2 + m.f03 * x3;
    r.xm[1] = x1 + m.f12 * x2 + m.f13 * x3;
    r.xm[2] = x2 + m.f23 * x3;
    r.xm[3] = x3;
    r.Pm = kf_fxft(m, s.P[l], i, j) + Q[l];
    const double hj2 = j == 0 ? m.h02 : m.h12, hj3 = j == 0 ? m.h03 : m.h13;
    r.M = r.Pm + hj2 * __shfl(r.Pm, 4 * i + 2) + hj3 * __shfl(r.Pm, 4 * i + 3);
    const double hi2 = i == 0 ? m.h02 : m.h12, hi3 = i == 0 ? m.h03 : m.h13;
    r.HP = r.Pm + hi2 * __shfl(r.Pm, 8 + j) + hi3 * __shfl(r.Pm, 12 + j);
    return r;
}

// The lane's row of the Kalman gain, K = M inv(H M + R) (:1162), and x = x- + K z (:1164)
[[maybe_unused]] __device__ __forceinline__ void kf_gain(const KfModel& m, const KfPred& p, const double (&R)[2], double z0, double z1, int lane,
    double (&K)[2], double (&xn)[4])
{
    const int l = lane & 15, i = l >> 2, j = l & 3;
    // S = (H P-) H^T + R, associated as the reference's expression is
    const double hj2 = j == 0 ? m.h02 : m.h12, hj3 = j == 0 ? m.h03 : m.h13;
    const double rij = i == j ? (i == 0 ? R[0] : R[1]) : 0.0;
    const double s = p.HP + hj2 * __shfl(p.HP, 4 * i + 2) + hj3 * __shfl(p.HP, 4 * i + 3) + rij;  // lanes 0, 1, 4, 5
    const double s00 = lane_d(s, 0), s01 = lane_d(s, 1), s10 = lane_d(s, 4), s11 = lane_d(s, 5);
    const double det = s00 * s11 - s01 * s10;
    const double v00 = s11 / det, v01 = -s01 / det, v10 = -s10 / det, v11 = s00 / det;
    const double mi0 = __shfl(p.M, 4 * i), mi1 = __shfl(p.M, 4 * i + 1);
    K[0] = mi0 * v00 + mi1 * v10;
    K[1] = mi0 * v01 + mi1 * v11;
    const double kz = K[0] * z0 + K[1] * z1;
#pragma unroll
    for (int q = 0; q < 4; ++q) xn[q] = p.xm[q] + lane_d(kz, 4 * q);
}

// P(i, j) = ((I - K H) P-)(i, j) (:1166): the lane's row of I - K H times its column of P-
[[maybe_unused]] __device__ __forceinline__ double kf_cov(const KfModel& m, const KfPred& p, const double (&K)[2], int lane)
{
    const int l = lane & 15, i = l >> 2, j = l & 3;
    const double g0 = (i == 0 ? 1.0 : 0.0) - K[0];
    const double g1 = (i == 1 ? 1.0 : 0.0) - K[1];
    const double g2 = (i == 2 ? 1.0 : 0.0) - (K[0] * m.h02 + K[1] * m.h12);
    const double g3 = (i == 3 ? 1.0 : 0.0) - (K[0] * m.h03 + K[1] * m.h13);
    return g0 * __shfl(p.Pm, j) + g1 * __shfl(p.Pm, 4 + j) + g2 * __shfl(p.Pm, 8 + j) + g3 * __shfl(p.Pm, 12 + j);
}

struct KfSpec  // wave 1's filter step of a call, as far as wave 0's loop update needs it
{
    double code_error_kf_chips, carrier_phase_kf_rad, carrier_doppler_kf_hz;
    double R[2];
    float log_err[4];
};

// The Kalman loop's LDS: x / P in two slots (wave 1 steps from the current one into the
// other, wave 0 switches when the call stays locked), d_Q, d_R's diagonal and wave 1's
// results; 528 bytes, allocated for the KF kernel instances only
struct KfShared
{
    KfSlot slot[2];
    double q[16], r[2];
    KfSpec spec;
    int cur;
};

template <bool KF>
struct KfWave0  // wave 0's locals of a call in the Kalman loop; none in the DLL/PLL kernels
{
};

template <bool KF>
__device__ __forceinline__ KfShared* kf_shared()
{
    if constexpr (KF)
        {
            __shared__ KfShared s;
            return &s;
        }
    else
        return nullptr;
}

struct KfLink  // the Kalman loop's SpecLink (take_kf, kf_narrow)
{
    const KfSpec* res;   // LDS: wave 1's filter step of the call
    int* ready;          // LDS: the call index whose step res holds
    double* kfq;         // LDS: d_Q
    const Cn0Spec* cn0;  // LDS: wave 2's lock test of the call
    int* cn0_e;
    int kfi;             // wave 0: the current x / P slot
    int e;               // wave 0: this call's index
    double R[2];         // wave 0: the call's d_R, stored when the call stays locked
};

template <>
struct KfWave0<true>
{
    int kfi0;   // the x / P slot current at the call's start
    KfLink kl;
};

// The rest of run_Kf (:1168-1203) from wave 1's filter step: the NCO commands
[[maybe_unused]] __device__ inline void take_kf(const TrkConst& c, TrkHot& t, KfLink& sl)
{
    while (__hip_atomic_load(sl.ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != sl.e)
        __builtin_amdgcn_s_sleep(1);
    const KfSpec r = *sl.res;
    t.carrier_doppler_hz = r.carrier_doppler_kf_hz;
    t.P_accu_old = t.P_accu;
    t.code_freq_chips = c.code_chip_rate + r.carrier_doppler_kf_hz * c.code_chip_rate / c.signal_carrier_freq;
    t.rem_code_phase_samples += c.fs_in * r.code_error_kf_chips / t.code_freq_chips;
    t.rem_carr_phase_rad = (float)r.carrier_phase_kf_rad;
    for (int i = 0; i < 4; ++i) t.log_err[i] = r.log_err[i];
    sl.R[0] = r.R[0];
    sl.R[1] = r.R[1];
    sl.kfi ^= 1;  // wave 1 stepped into the other slot
}

// update_kf_narrow_integration_time (:898-935) at the switch to the extended correlator:
// d_Q summed over extend_correlation_symbols steps of the old d_F (d_Q itself replaced
// in the loop), d_R from this call's C/N0 with the new Ti and the still wide spc; d_F and
// d_H follow t.corr_time.  Once per channel, on wave 0's lanes like the per-call algebra.
[[maybe_unused]] __device__ inline void kf_narrow(const TrkConst& c, const TrkHot& t, KfLink& sl, double Ti_old, int lane)
{
    const int l = lane & 15, i = l >> 2, j = l & 3;
    // the branch this runs in is void on a loss of lock (the caller rebuilds the call):
    // nothing is written then
    while (__hip_atomic_load(sl.cn0_e, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != sl.e)
        __builtin_amdgcn_s_sleep(1);
    if (!sl.cn0->locked) return;
    const KfModel m = kf_model(c.kf_beta, Ti_old);
    double q = sl.kfq[l], qnew = 0.0;
    for (int n = 0; n < c.extend_correlation_symbols; ++n)
        {
            q = kf_fxft(m, q, i, j);
            qnew += q;
        }
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) sl.kfq[lane] = qnew;
    kf_r_of_cn0(sl.cn0->cn0_db_hz, t.corr_time, t.spc, sl.R);
}

}  // namespace
