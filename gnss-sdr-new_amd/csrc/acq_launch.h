// Launch templates of the acquisition engine over the FFT plan type, and the
// per-plan dispatch of an AcqOp.  Included only by the acq_v_*.hip units, each of
// which instantiates them for one group of acq_plans.h.
#pragma once
#include "acq_handle.h"
#include "acq_iqcaf_kernels.h"
#include "acq_plans.h"
#include "acq_quicksync_kernels.h"
#include "acq_tong_kernels.h"

namespace
{
using namespace gsdr_acq_impl;

template <class PT>
int set_lds_attrs(size_t bytes)
{
    const void* const kernels[] = {(const void*)acq_code_fft_kernel<PT>, (const void*)acq_correlate_kernel<PT, false>,
        (const void*)acq_correlate_kernel<PT, true>, (const void*)acq_second_peak_kernel<PT>,
        (const void*)acq_correlate_dwell_kernel<PT>, (const void*)acq_second_peak_dwell_kernel<PT>,
        (const void*)acq_dwell_grid_kernel<PT>};
    int rc = GSDR_OK;
    for (const void* k : kernels) rc |= set_max_lds(k, bytes);
    for (int it : kItemTypes)
        rc |= with_item_type(it, [&](auto t) {
            return set_max_lds((const void*)acq_forward_kernel<PT, decltype(t)::value>, bytes);
        });
    if constexpr (!std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        for (int it : kItemTypes)
            rc |= with_item_type(it, [&](auto t) {
                return set_max_lds((const void*)acq_forward_fold_kernel<PT, decltype(t)::value>, bytes);
            });
    if constexpr (std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        {
            rc |= set_max_lds((const void*)acq_argmax_four_kernel<PT>, bytes);
            rc |= set_max_lds((const void*)acq_argmax_second_four_kernel<PT>, bytes);
            if constexpr (requires_subplan<PT>::value)
                rc |= set_max_lds((const void*)acq_forward4_rows_kernel<PT>, PT::SubPlan::lds_bytes());
        }
    return rc == GSDR_OK ? GSDR_OK : GSDR_E_DEVICE;
}

// The plan object a plan type's kernels take (LDS plan or four-step plan).
template <class PT>
const typename PT::PlanT& plan_of(const gsdr_acq* a)
{
    if constexpr (std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        return a->plan4;
    else
        return a->plan;
}

template <class PT>
void launch_forward(gsdr_acq* a, const AcqView& v, const void* iq, uint32_t nblocks, uint64_t stride, hipStream_t s)
{
    // a folding view (LDS plans only; QuickSync, acq_quicksync.hip): items of fold_segments N
    // samples at stride, v.wipe their rows, folded by the load
    if constexpr (!std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        if (v.fold_segments > 0)
            {
                with_item_type(a->conf.item_type, [&](auto t) {
                    hipLaunchKernelGGL((acq_forward_fold_kernel<PT, decltype(t)::value>), dim3(nblocks, v.xm.q),
                        dim3(PT::NT), a->lds_bytes, s, iq, stride, v.wipe, a->d_X, a->d_tw, plan_of<PT>(a),
                        v.fold_segments, v.xm);
                });
                return;
            }
    with_item_type(a->conf.item_type, [&](auto t) {
        hipLaunchKernelGGL((acq_forward_kernel<PT, decltype(t)::value>), dim3(nblocks, v.xm.q), dim3(PT::NT),
            a->lds_bytes, s, iq, stride, v.wipe, a->d_X, a->d_tw, plan_of<PT>(a), a->consumed, v.xm);
    });
}

// The two-launch forward (acq_forward4_cols_kernel + acq_forward4_rows_kernel).
template <class PT>
void launch_forward_two(gsdr_acq* a, const AcqView& v, const void* iq, uint32_t nblocks, uint64_t stride, hipStream_t s)
{
    // the xm.q stored spectra per block (XMap): rows b * q + d, d < q
    const uint32_t nrows = nblocks * v.xm.q;
    const dim3 cg((PT::N2 + 255) / 256, nrows);
    with_item_type(a->conf.item_type, [&](auto t) {
        hipLaunchKernelGGL((acq_forward4_cols_kernel<PT, decltype(t)::value>), cg, dim3(256), 0, s, iq, stride, v.wipe,
            a->d_fscratch, a->d_tw, a->consumed, v.xm.q);
    });
    hipLaunchKernelGGL((acq_forward4_rows_kernel<PT>), dim3(nrows * PT::R), dim3(PT::NT), PT::SubPlan::lds_bytes(), s,
        a->d_fscratch, a->d_X, a->d_tw_sub, nrows, v.xm.stride);
}

// General path (max_dwells > 1 and/or bit_transition_flag): forward spectra of
// all nblocks*K blocks, the dwell-accumulating correlate kernel, per-dwell
// statistics and the dwell decision.
template <class PT>
int launch_general(gsdr_acq* a, const AcqView& v, const AcqOp& op, StageTimer& t)
{
    const size_t lds = a->lds_bytes;
    const uint32_t K = a->K, nblocks = op.nblocks;
    hipStream_t s = op.s;
    t.begin();
    launch_forward<PT>(a, v, op.iq, nblocks * K, op.stride, s);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    const AcqParams ap = params_of(a, v);
    t.begin();
    hipLaunchKernelGGL((acq_correlate_dwell_kernel<PT>), dim3(v.D * v.nprn * nblocks), dim3(PT::NT), lds, s, a->d_X,
        v.code_fft, a->d_stats, a->d_tw, plan_of<PT>(a), ap, a->d_acc, a->d_acc_slots, a->acc_words);
    GSDR_HIP(hipGetLastError());
    t.end(1);
    t.begin();
    int rc = launch_reduce(a, ap, true, nblocks, op.res, v.prn, op.stamp0, op.stride, s);
    if (rc != GSDR_OK) return rc;
    t.end(2);
    if (!ap.cfar)
        {
            t.begin();
            hipLaunchKernelGGL((acq_second_peak_dwell_kernel<PT>), dim3(K, nblocks * v.nprn), dim3(PT::NT), lds, s,
                a->d_X, v.code_fft, a->d_resk, a->d_tw, plan_of<PT>(a), ap, a->d_acc, a->d_acc_slots, a->acc_words);
            GSDR_HIP(hipGetLastError());
            rc = launch_decide(a, nblocks * v.nprn, op.res, s);
            if (rc != GSDR_OK) return rc;
            t.end(3);
        }
    return GSDR_OK;
}

// Split register four-step path (single dwell, with or without bit transition):
// forward spectra on PT, the split correlate's row maxima, the grid maximum, the
// selected row recomputed (on the split plan, or on PT) for the first-maximum index /
// exact peak / CFAR power, and (peak ratio) the second peak on the same row.
template <class PT>
int launch_split_all(gsdr_acq* a, const AcqView& v, const AcqOp& op, StageTimer& t)
{
    const size_t lds = a->lds_bytes;
    const uint32_t nblocks = op.nblocks;
    gsdr_acq_result* res = op.res;
    hipStream_t s = op.s;
    t.begin();
    if constexpr (requires_subplan<PT>::value)
        {
            if (a->d_fscratch)
                launch_forward_two<PT>(a, v, op.iq, nblocks, op.stride, s);
            else
                launch_forward<PT>(a, v, op.iq, nblocks, op.stride, s);
        }
    else
        launch_forward<PT>(a, v, op.iq, nblocks, op.stride, s);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    const AcqParams ap = params_of(a, v);
    t.begin();
    int rc = launch_split(a, v, nblocks, s);
    if (rc != GSDR_OK) return rc;
    t.end(1);
    t.begin();
    rc = launch_reduce(a, ap, false, nblocks, res, v.prn, op.stamp0, op.stride, s);
    if (rc != GSDR_OK) return rc;
    // the selected rows on the split plan itself (AcqEnv::split_arg off: recomputed on PT);
    // CFAR with bit transition needs the opposite row's half window: recomputed on PT
    if (a->env.split_arg && a->d_keys && !(ap.cfar && a->eff != a->N) && (ap.cfar || a->d_rowbuf))
        {
            rc = launch_split_argmax(a, v, nblocks, res, s);
            if (rc != GSDR_OK) return rc;
        }
    else if (ap.cfar || !a->d_rowbuf)
        {
            hipLaunchKernelGGL((acq_argmax_four_kernel<PT>), dim3(nblocks * v.nprn), dim3(PT::NT), lds, s, a->d_X,
                v.code_fft, res, a->d_tw, plan_of<PT>(a), ap);
            GSDR_HIP(hipGetLastError());
        }
    else
        {
            // peak ratio: first and second peak from one recomputation of the row
            hipLaunchKernelGGL((acq_argmax_second_four_kernel<PT>), dim3(nblocks * v.nprn), dim3(PT::NT), lds, s,
                a->d_X, v.code_fft, res, a->d_tw, plan_of<PT>(a), ap, a->d_rowbuf);
            GSDR_HIP(hipGetLastError());
        }
    t.end(2);
    if (!ap.cfar && !a->d_rowbuf)
        {
            t.begin();
            hipLaunchKernelGGL((acq_second_peak_kernel<PT>), dim3(nblocks * v.nprn), dim3(PT::NT), lds, s, a->d_X,
                v.code_fft, res, a->d_tw, plan_of<PT>(a), ap);
            GSDR_HIP(hipGetLastError());
            t.end(3);
        }
    return GSDR_OK;
}

template <class PT>
int launch_all(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    const size_t lds = a->lds_bytes;
    const uint32_t nblocks = op.nblocks;
    gsdr_acq_result* res = op.res;
    hipStream_t s = op.s;
    StageTimer t(a, s);
    if constexpr (std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
        {
            if (a->split > 0) return launch_split_all<PT>(a, v, op, t);
        }
    if (a->general) return launch_general<PT>(a, v, op, t);
    t.begin();
    if (a->corr_variant > 0)
        {
            int rc = launch_forward_pk(a, v, op.iq, nblocks, op.stride, s);
            if (rc != GSDR_OK) return rc;
        }
    else
        launch_forward<PT>(a, v, op.iq, nblocks, op.stride, s);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    t.begin();
    if (a->corr_variant > 0)
        {
            int rc = launch_corr_variant(a, v, nblocks, s);
            if (rc != GSDR_OK) return rc;
        }
    else
        {
            hipLaunchKernelGGL((acq_correlate_kernel<PT, false>), dim3(v.D * v.nprn, nblocks), dim3(PT::NT), lds, s,
                a->d_X, v.code_fft, a->d_stats, (float*)nullptr, a->d_tw, plan_of<PT>(a), v.D, v.nprn, 0u, v.xm);
        }
    GSDR_HIP(hipGetLastError());
    t.end(1);
    const AcqParams ap = params_of(a, v);
    t.begin();
    int rc = launch_reduce(a, ap, false, nblocks, res, v.prn, op.stamp0, op.stride, s);
    if (rc != GSDR_OK) return rc;
    if (a->corr_variant > 0 && a->corr_stat >= 1)
        {
            rc = launch_argmax_variant(a, v, nblocks, res, s);
            if (rc != GSDR_OK) return rc;
        }
    t.end(2);
    if (!ap.cfar)
        {
            t.begin();
            hipLaunchKernelGGL((acq_second_peak_kernel<PT>), dim3(nblocks * v.nprn), dim3(PT::NT), lds, s, a->d_X,
                v.code_fft, res, a->d_tw, plan_of<PT>(a), ap);
            GSDR_HIP(hipGetLastError());
            t.end(3);
        }
    return GSDR_OK;
}

// gsdr_acq_run_dwell: forward spectra of the block at a->d_iq, the accumulating
// grid kernel, the statistic with counter dwell+1 and (peak ratio) the second
// peak on the accumulated row.
template <class PT>
int launch_dwell(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    hipStream_t s = op.s;
    launch_forward<PT>(a, v, a->d_iq, 1, a->consumed, s);
    GSDR_HIP(hipGetLastError());
    AcqParams ap = params_of(a, v);
    ap.counter = op.dwell + 1;
    hipLaunchKernelGGL((acq_dwell_grid_kernel<PT>), dim3(v.D * v.nprn), dim3(PT::NT), a->lds_bytes, s, a->d_X,
        v.code_fft, a->d_stats, a->d_tw, plan_of<PT>(a), ap, a->d_dgrid, op.dwell);
    GSDR_HIP(hipGetLastError());
    const int rc = launch_reduce(a, ap, false, 1, op.res, v.prn, op.stamp0, (uint64_t)a->consumed, s);
    if (rc != GSDR_OK || ap.cfar) return rc;
    return launch_grid_second_peak(a, ap, op.res, s);
}

// Whether a plan type's Tong grid kernel is built with the running row in LDS, in HBM or both:
// a compile-time plan knows its size.
template <class PT>
constexpr bool tong_may_row_lds()
{
    return PT::N == 0 || (size_t)PT::N * (sizeof(float2) + sizeof(float)) + 16 * sizeof(RowStat) <= kLdsBytes;
}
template <class PT>
constexpr bool tong_may_row_hbm()
{
    return PT::N == 0 || !tong_may_row_lds<PT>();
}

template <class PT>
int set_tong_attrs(const gsdr_acq* a)
{
    int rc = GSDR_OK;
    if constexpr (tong_may_row_lds<PT>())
        if (tong_row_fits_lds(a)) rc |= set_max_lds((const void*)acq_tong_grid_kernel<PT, true>, tong_lds_bytes(a));
    if constexpr (tong_may_row_hbm<PT>())
        if (!tong_row_fits_lds(a)) rc |= set_max_lds((const void*)acq_tong_grid_kernel<PT, false>, tong_lds_bytes(a));
    return rc == GSDR_OK ? GSDR_OK : GSDR_E_DEVICE;
}

// gsdr_acq_run_tong: forward spectra of the nblocks items at op.iq and the grid kernel over
// them on the view's Tong buffers.
template <class PT>
int launch_tong(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    hipStream_t s = op.s;
    StageTimer t(a, s);
    t.begin();
    launch_forward<PT>(a, v, op.iq, op.nblocks, op.stride, s);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    t.begin();
    if constexpr (tong_may_row_lds<PT>())
        if (v.tong_row_lds)
            hipLaunchKernelGGL((acq_tong_grid_kernel<PT, true>), dim3(v.D * v.nprn), dim3(PT::NT), tong_lds_bytes(a), s,
                a->d_X, v.code_fft, v.tong_stats, a->d_tw, plan_of<PT>(a), v.tong_grid, v.tong_scale, v.tong_slots, v.D,
                v.nprn, op.nblocks, v.xm);
    if constexpr (tong_may_row_hbm<PT>())
        if (!v.tong_row_lds)
            hipLaunchKernelGGL((acq_tong_grid_kernel<PT, false>), dim3(v.D * v.nprn), dim3(PT::NT), tong_lds_bytes(a), s,
                a->d_X, v.code_fft, v.tong_stats, a->d_tw, plan_of<PT>(a), v.tong_grid, v.tong_scale, v.tong_slots, v.D,
                v.nprn, op.nblocks, v.xm);
    GSDR_HIP(hipGetLastError());
    t.end(1);
    return GSDR_OK;
}

// The IQ-CAF grid kernel's LDS attribute for the handle's settings (gsdr_acq_set_iq_caf).
template <class PT>
int set_iqcaf_attrs(const gsdr_acq* a)
{
    const size_t bytes = iqcaf_lds_bytes(a, a->iq.nslots, a->iq.rows_lds);
    return a->iq.rows_lds ? set_max_lds((const void*)acq_iqcaf_grid_kernel<PT, true>, bytes)
                          : set_max_lds((const void*)acq_iqcaf_grid_kernel<PT, false>, bytes);
}

// gsdr_acq_run_iq_caf: forward spectra of the nblocks items at op.iq -- the engine's own forward
// pass, in two launches where the split path has its scratch -- and the grid kernel over them on
// the view's IQ-CAF buffers, one workgroup per (row, satellite, item).
template <class PT>
int launch_iqcaf(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    hipStream_t s = op.s;
    StageTimer t(a, s);
    t.begin();
    bool two = false;
    if constexpr (requires_subplan<PT>::value) two = a->d_fscratch != nullptr;
    if constexpr (requires_subplan<PT>::value)
        {
            if (two) launch_forward_two<PT>(a, v, op.iq, op.nblocks, op.stride, s);
        }
    if (!two) launch_forward<PT>(a, v, op.iq, op.nblocks, op.stride, s);
    GSDR_HIP(hipGetLastError());
    t.end(0);
    t.begin();
    const uint32_t nsat = v.nprn / v.iq_nslots;
    const dim3 grid(v.D * nsat, op.nblocks);
    const size_t lds = iqcaf_lds_bytes(a, v.iq_nslots, v.iq_rows_lds);
    if (v.iq_rows_lds)
        hipLaunchKernelGGL((acq_iqcaf_grid_kernel<PT, true>), grid, dim3(PT::NT), lds, s, a->d_X, v.code_fft, v.iq_rec,
            a->d_tw, plan_of<PT>(a), (float*)nullptr, v.D, nsat, v.iq_nslots, v.iq_both ? 1u : 0u, v.xm);
    else
        hipLaunchKernelGGL((acq_iqcaf_grid_kernel<PT, false>), grid, dim3(PT::NT), lds, s, a->d_X, v.code_fft, v.iq_rec,
            a->d_tw, plan_of<PT>(a), v.iq_rows, v.D, nsat, v.iq_nslots, v.iq_both ? 1u : 0u, v.xm);
    GSDR_HIP(hipGetLastError());
    t.end(1);
    return GSDR_OK;
}

// Code spectra of slots [first_slot, first_slot + nslots) from their staged codes.
template <class PT>
int launch_code_fft(gsdr_acq* a, const AcqOp& op)
{
    hipLaunchKernelGGL((acq_code_fft_kernel<PT>), dim3(op.nslots), dim3(PT::NT), a->lds_bytes, a->stream,
        a->d_code_stage + (size_t)op.first_slot * a->consumed, a->d_code_fft + (size_t)op.first_slot * a->N, a->d_tw,
        plan_of<PT>(a), a->consumed, a->lead);
    GSDR_HIP(hipGetLastError());
    return GSDR_OK;
}

// Forward spectra of the block at a->d_iq and (grid) the |R|^2 rows of one PRN slot.
template <class PT>
int launch_dump(gsdr_acq* a, const AcqView& v, bool grid, uint32_t prn_slot)
{
    launch_forward<PT>(a, v, a->d_iq, 1, a->consumed, a->stream);
    GSDR_HIP(hipGetLastError());
    if (grid)
        {
            hipLaunchKernelGGL((acq_correlate_kernel<PT, true>), dim3(v.D, 1), dim3(PT::NT), a->lds_bytes, a->stream,
                a->d_X, v.code_fft, a->d_stats, a->d_grid, a->d_tw, plan_of<PT>(a), v.D, v.nprn, prn_slot, v.xm);
            GSDR_HIP(hipGetLastError());
        }
    return GSDR_OK;
}

template <class PT>
int run_op(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    switch (op.kind)
        {
        case AcqOp::Run: return launch_all<PT>(a, v, op);
        case AcqOp::CodeFft: return launch_code_fft<PT>(a, op);
        case AcqOp::DumpSpectra: return launch_dump<PT>(a, v, false, 0);
        case AcqOp::DumpGrid: return launch_dump<PT>(a, v, true, op.prn_slot);
        case AcqOp::Dwell: return launch_dwell<PT>(a, v, op);
        case AcqOp::SetAttrs:
            {
                const int rc = set_lds_attrs<PT>(a->lds_bytes);
                if constexpr (!std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
                    if (rc == GSDR_OK) return set_tong_attrs<PT>(a);
                return rc;
            }
        case AcqOp::Tong:
            // LDS plans only (gsdr_acq_set_tong refuses the four-step sizes)
            if constexpr (!std::is_same<typename PT::PlanT, gsdr::fft::Plan4>::value)
                return launch_tong<PT>(a, v, op);
            else
                break;
        case AcqOp::IqCaf: return launch_iqcaf<PT>(a, v, op);
        case AcqOp::IqCafAttrs: return set_iqcaf_attrs<PT>(a);
        }
    return GSDR_E_STATE;
}

// The op on the plan of the list that the handle's variant names.
template <class List>
int run_on(List plans, gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    int rc = GSDR_E_STATE;
    const bool found = find_plan(plans, [&](auto e) {
        if (decltype(e)::id != a->variant) return false;
        rc = run_op<typename decltype(e)::type>(a, v, op);
        return true;
    });
    if (!found) gsdr::set_error("internal: bad FFT variant %d", a->variant);
    return rc;
}

}  // namespace
