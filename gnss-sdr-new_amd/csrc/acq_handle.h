// Host side shared by the acquisition translation units: the handle, the view a
// launch runs on, the typed operation of the per-plan dispatch, and the host
// helpers and launch functions each defined in one unit.
#pragma once
#include <mutex>
#include <type_traits>
#include <vector>

#include "acq_kernels.h"
#include "gsdr_stream_internal.h"

// Runtime switches, read once per handle by read_acq_env (acq_common.hip, which
// documents each of them).
struct AcqEnv
{
    int wipe_mode{GSDR_WIPE_EXACT};
    bool xshift{true}, four_generic{false}, split{true}, split_arg{true};
    int qpw{0}, ppw{0};
    int corr_variant{-1};  // -1: default_pk_variant(N)
    bool iqcaf_rows_hbm{false};
};

// ====================================================================== handle
struct gsdr_acq
{
    int device{0};
    gsdr_acq_conf conf{};
    AcqEnv env{};
    uint32_t N{0}, D{0}, consumed{0}, lead{0};
    uint32_t K{1};       // max_dwells
    int wipe_mode{GSDR_WIPE_EXACT};  // carrier model of the Doppler grid (gsdr_acq_set_wipeoff)
    gsdr_acq_impl::XMap xm{};  // forward-spectrum layout of the main Doppler grid (rebuild_wipeoffs)
    uint32_t eff{0};     // effective FFT size (outputs [N - eff, N))
    bool general{false}; // dwells > 1 or bit transition: the general kernels
    gsdr_acq_result* d_resk{nullptr};  // per-dwell results (general path)
    float* d_acc{nullptr};             // pooled |R|^2 accumulation rows (general path)
    uint32_t* d_acc_slots{nullptr};
    int acc_words{0};
    float threshold{0.0f};
    int nt{256};
    int variant{0};           // FFT plan id (acq_plans.h)
    int corr_variant{0};      // 0: the generic LDS kernels; >0: a PkVariants id (packed forward + correlate, acq_pk.hip)
    int split{0};             // >0: the single-dwell split register four-step correlate (acq_split.hip)
    int corr_stat{0};         // the variant's row statistic (1/2: argmax recomputed by acq_argmax_pk_kernel)
    size_t corr_lds_bytes{0};
    int lane_nb1{0}, lane_r1{0};  // the variant's correlate reads d_code_lane: its first stage's butterflies and radix
    int lane_pfa{0};              // ... in the prime-factor plan's order (pfa_lane_order_slot) instead of lane_order_slot
    gsdr::fft::Plan plan{};
    gsdr::fft::Plan4 plan4{};  // four-step plan (variants 20-27, N beyond one workgroup's LDS)
    size_t lds_bytes{0};
    hipStream_t stream{nullptr};
    float2* d_tw{nullptr};
    float2* d_wipe{nullptr};
    float2* d_code_fft{nullptr};
    float2* d_code_lane{nullptr};  // the same rows in first-stage lane order (lane_order_slot / lane_pfa), variants with lane_nb1 > 0
    float2* d_code_stage{nullptr};
    uint32_t* d_prn{nullptr};
    uint32_t nprn{0};
    // what the nprn active code slots hold (set_slots, called by every code setter):
    // plain codes, nprn / 2 pairs, nprn folded QuickSync codes or iq.nslots slots per IQ-CAF satellite
    enum class Slots
    {
        Plain,
        Pairs,
        QuickSync,
        IqCaf
    } slots{Slots::Plain};
    float2* d_X{nullptr};
    gsdr_acq_impl::RowStat* d_stats{nullptr};
    gsdr_acq_result* d_res{nullptr};
    // gsdr_acq_submit_stream / gsdr_acq_collect: up to kSubs submissions in flight,
    // each with its pinned results (max_blocks x max_prns), completion event and shape;
    // a later submission's grid reuses d_res on the same stream, ordered after the
    // earlier one's copy out of it
    static constexpr int kSubs = 2;
    gsdr_acq_result* h_res[kSubs]{};
    hipEvent_t sub_done[kSubs]{};
    uint32_t sub_blocks[kSubs]{}, sub_nprn[kSubs]{};
    int sub_head{0}, sub_count{0};
    void* d_iq{nullptr};
    float* d_grid{nullptr};
    float* d_rowbuf{nullptr};  // split path, peak ratio: the selected rows' |R|^2 (max_blocks x max_prns x N)
    unsigned long long* d_keys{nullptr};  // split path: the selected rows' first-maximum keys (max_blocks x max_prns)
    float* d_psum{nullptr};               // split path, CFAR: Parseval shares per sub-transform (max_blocks x max_prns x 4)
    float2* d_fscratch{nullptr};  // split path: the two-launch forward's column-DFT rows (max_blocks x D x N)
    float* d_dgrid{nullptr};     // gsdr_acq_run_dwell: the |R|^2 grid kept across calls (max_prns x D x eff)
    float2* d_tw_sub{nullptr};   // four-step: W_N2 table
    float2* d_scratch{nullptr};  // four-step: slot rows of N complex
    uint32_t* d_slots{nullptr};  // four-step: slot occupancy bitmap
    // stage profiling (gsdr_acq_set_profiling)
    struct ProfRec
    {
        hipEvent_t a, b;
        int stage;
    };
    bool profiling{false};
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    // make_two_steps (gsdr_acq_set_step_two / gsdr_acq_run_step_two)
    struct StepTwo
    {
        uint32_t nbins{0};       // num_doppler_bins_step2
        float step{0.0f};        // doppler_step2
        float pfa2{0.0f};
        float2* d_wipe{nullptr}; // max_prns x nbins rows of N
        float* d_freq{nullptr};
    } st2;
    // fine-Doppler estimate (gsdr_acq_fine_doppler, acq_fine.hip): the L = 10 N point
    // plan, its tables and scratch pool, built on the first call (or at create with
    // GSDR_ACQ_FINE=1), and the per-call buffers, grown on demand
    struct Fine
    {
        bool ready{false};
        uint32_t L{0};
        int r1{0};  // 0: one LDS plan; else the four-step's register radix (L = r1 * n2)
        int nt{0};
        gsdr::fft::Plan plan{};
        gsdr::fft::Plan4 plan4{};
        size_t lds_bytes{0};
        float2* d_tw{nullptr};       // W_L
        float2* d_tw_sub{nullptr};   // four-step: W_N2
        float2* d_scratch{nullptr};  // four-step: kFineSlots rows of L complex
        uint32_t* d_slots{nullptr};
        void* d_iq{nullptr};         // the 10 ms window of the host forms
        float2* d_codes{nullptr};
        uint32_t codes_cap{0};
        gsdr_acq_fine_request* d_req{nullptr};
        gsdr_acq_fine_result* d_out{nullptr};
        unsigned long long* d_keys{nullptr};
        uint32_t req_cap{0};
        float* d_spec{nullptr};      // gsdr_acq_dump_fine_spectrum: 80 N floats
    } fine;
    // paired-code acquisition (gsdr_acq_set_code_pairs / gsdr_acq_run_pairs, acq_pair.hip):
    // pair q holds code slots 2 q and 2 q + 1; the buffers are built by the first
    // gsdr_acq_set_code_pairs
    struct Pairs
    {
        float2* d_in{nullptr};    // the caller's two arguments: 2 x (max_prns / 2) rows of N
        float* d_power{nullptr};  // max_blocks input powers
        gsdr_acq_pair_result* d_out{nullptr};  // max_blocks x (max_prns / 2) records
    } pairs;
    // QuickSync acquisition (gsdr_acq_set_quicksync / gsdr_acq_run_quicksync, acq_quicksync.hip):
    // the handle's fft_size is Nf = spc / p; the buffers are built by gsdr_acq_set_quicksync
    struct Quick
    {
        uint32_t p{0};            // folding factor (> 0: configured)
        uint32_t spc{0};          // samples per code (p Nf); an item is L = p spc samples
        void* d_iq{nullptr};      // host items' staging: max_blocks x L items of the handle's type
        float2* d_wipe{nullptr};  // D rows (xm.q with the spectrum reuse) of L
        float2* d_codes{nullptr}; // max_prns unfolded codes of spc
        float* d_power{nullptr};  // max_blocks input powers
        float* d_cand{nullptr};   // max_blocks x max_prns x p candidate powers
        gsdr_acq_quicksync_result* d_out{nullptr};  // max_blocks x max_prns records
    } qs;
    // Tong acquisition (gsdr_acq_set_tong / gsdr_acq_run_tong, acq_tong.hip): the buffers are
    // built by gsdr_acq_set_tong
    struct Tong
    {
        uint32_t init{0}, max{0}, max_dwells{0};  // tong_init_val, tong_max_val (> 0: configured), tong_max_dwells
        bool row_lds{false};  // the grid kernel keeps its running row in LDS beside the transform's buffer
        float* d_grid{nullptr};   // max_prns x D x N accumulated rows
        gsdr_acq_impl::TongSlot* d_slots{nullptr};  // max_prns sequence states
        float* d_power{nullptr};  // max_blocks input powers
        float* d_scale{nullptr};  // max_blocks scales 1 / (fn fn P_k)
        gsdr_acq_impl::RowStat* d_stats{nullptr};   // max_blocks x max_prns x D row maxima of the accumulated rows
        gsdr_acq_tong_result* d_out{nullptr};       // max_blocks x max_prns records
    } tong;
    // E5a non-coherent IQ acquisition with CAF filter (gsdr_acq_set_iq_caf / gsdr_acq_run_iq_caf,
    // acq_iqcaf.hip): the buffers are built by gsdr_acq_set_iq_caf
    struct IqCaf
    {
        uint32_t nslots{0};  // code slots per satellite: 1, 2 or 4 (> 0: configured)
        uint32_t spc{0}, coherent_ms{0};
        bool both{false};
        int32_t window_hz{0};
        bool rows_lds{false};  // the grid kernel keeps a workgroup's |.|^2 rows in LDS
        float2* d_in{nullptr};    // the caller's rows: 2 x (max_prns / nslots) rows of N
        float* d_rows{nullptr};   // rows in HBM: max_blocks x (max_prns / nslots) x D regions of nslots x N
        float* d_power{nullptr};  // max_blocks input powers
        gsdr_acq_iq_caf_row* d_rec{nullptr};     // max_blocks x (max_prns / nslots) x D row records
        gsdr_acq_iq_caf_result* d_out{nullptr};  // max_blocks x (max_prns / nslots) records
    } iq;
    std::mutex mu;
};

namespace gsdr_acq_impl
{

// What a launch runs on: the Doppler rows, PRNs and spectrum layout in effect, and the
// mode of the run.  Built from the handle at the top of each ABI call (view_of); step
// two builds a one-PRN view over its narrow rows, and a pair or QuickSync run sets its
// mode on its own view, instead of altering the handle.  The launch functions read the
// mode here, never on the handle.
struct AcqView
{
    uint32_t D{0}, nprn{0};
    const float2* wipe{nullptr};      // D wipe-off rows (xm.q of them with the spectrum reuse)
    const float2* code_fft{nullptr};  // nprn code spectra
    const float2* code_lane{nullptr}; // the same rows in lane order (null unless the handle keeps them)
    const uint32_t* prn{nullptr};     // their PRN ids
    XMap xm{};
    // make_two_steps narrow grid (AcqParams::step_two ...)
    bool step_two{false};
    float center2{0.0f}, ip2{0.0f}, threshold2{0.0f};
    // > 0: the forward pass folds that many segments per point (QuickSync's p^2, LDS and
    // packed plans only); the items are op.stride apart and wipe holds rows over an item
    uint32_t fold_segments{0};
    // the CFAR launch sequence whatever conf.pfa says: its reduce and selected-row passes
    // give each slot's maximum, row and first index, and no second-peak pass follows
    bool first_peak_only{false};
    // a Tong run (AcqOp::Tong, acq_tong.hip): the accumulated grid, the items' scales, the
    // slots' sequence states, where the row maxima go and where the running row is kept
    float* tong_grid{nullptr};
    const float* tong_scale{nullptr};
    const TongSlot* tong_slots{nullptr};
    RowStat* tong_stats{nullptr};
    bool tong_row_lds{false};
    // an IQ-CAF run (AcqOp::IqCaf, acq_iqcaf.hip): nprn = iq_nslots x satellites; the row
    // records, the HBM rows (null: the rows wait in LDS) and the slot layout
    gsdr_acq_iq_caf_row* iq_rec{nullptr};
    float* iq_rows{nullptr};
    uint32_t iq_nslots{0};
    bool iq_both{false}, iq_rows_lds{false};
};

// The operation of a per-plan dispatch, with the arguments each kind reads.
struct AcqOp
{
    enum Kind
    {
        Run,          // iq, nblocks, stride, stamp0, res, s
        CodeFft,      // first_slot, nslots
        DumpSpectra,  // (the block at d_iq)
        DumpGrid,     // prn_slot
        SetAttrs,
        Dwell,        // dwell, stamp0, res, s
        Tong,         // iq, nblocks, stride, s (the view's tong_* fields)
        IqCaf,        // iq, nblocks, stride, s (the view's iq_* fields)
        IqCafAttrs    // the LDS attribute of the IQ-CAF grid kernel for the handle's iq settings
    } kind;
    const void* iq{nullptr};
    uint32_t nblocks{0};
    uint64_t stride{0}, stamp0{0};
    gsdr_acq_result* res{nullptr};
    hipStream_t s{nullptr};
    uint32_t first_slot{0}, nslots{0}, prn_slot{0}, dwell{0};
};

// The LDS a workgroup of the engine may ask for (choose_variant, acq.hip).
constexpr size_t kLdsBytes = 160 * 1024;

// Dynamic LDS of acq_tong_grid_kernel on the handle's plan: with the running row of N floats
// behind the transform's buffer and the statistics scratch where that fits the limit.
inline bool tong_row_fits_lds(const gsdr_acq* a) { return a->lds_bytes + (size_t)a->N * sizeof(float) <= kLdsBytes; }
inline size_t tong_lds_bytes(const gsdr_acq* a)
{
    return a->lds_bytes + (tong_row_fits_lds(a) ? (size_t)a->N * sizeof(float) : 0);
}

// Dynamic LDS of acq_iqcaf_grid_kernel on the handle's plan: behind the transform's buffer and
// the statistics scratch a 64-byte stash of the slots' peaks, then the satellite's nslots rows of
// N floats where that fits the limit (the four-step plans keep a word of static LDS besides).
constexpr size_t kIqCafStash = 64;
inline bool iqcaf_rows_fit_lds(const gsdr_acq* a, uint32_t nslots)
{
    return !a->env.iqcaf_rows_hbm &&
           a->lds_bytes + kIqCafStash + (size_t)nslots * a->N * sizeof(float) + (a->variant >= 20 ? 16 : 0) <= kLdsBytes;
}
inline size_t iqcaf_lds_bytes(const gsdr_acq* a, uint32_t nslots, bool rows_lds)
{
    return a->lds_bytes + kIqCafStash + (rows_lds ? (size_t)nslots * a->N * sizeof(float) : 0);
}

// Default packed correlate variant for an FFT size (0: none, the generic kernels).
inline int default_pk_variant(uint32_t N)
{
    switch (N)
        {
        case 4000: return 103;  // 101 (prime-factor 32 x 125 plan) on the 16-instruction 5-point transform, |z|^2 of two outputs packed: +3 % over 101
        case 16000: return 94;  // r04a: wave-local rows, +3 % over 93
        case 8000: return 61;
        case 2000: return 62;
        default: return 0;
        }
}

// f(std::integral_constant<int, GSDR_ITEM_*>) for a runtime item type.
template <class F>
auto with_item_type(int it, F&& f)
{
    if (it == GSDR_ITEM_GR_COMPLEX) return f(std::integral_constant<int, GSDR_ITEM_GR_COMPLEX>{});
    if (it == GSDR_ITEM_CSHORT) return f(std::integral_constant<int, GSDR_ITEM_CSHORT>{});
    return f(std::integral_constant<int, GSDR_ITEM_IBYTE>{});
}
constexpr int kItemTypes[] = {GSDR_ITEM_GR_COMPLEX, GSDR_ITEM_CSHORT, GSDR_ITEM_IBYTE};

// The one statement of what the code slots hold, for the code setters.
inline void set_slots(gsdr_acq* a, gsdr_acq::Slots kind, uint32_t nprn)
{
    a->slots = kind;
    a->nprn = nprn;
}

inline int set_max_lds(const void* kernel, size_t bytes)
{
    GSDR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return GSDR_OK;
}

// Event bracket around one stage launch when profiling is on (gsdr_acq_set_profiling): a
// record owns its two events, taken from the handle's pool.
struct StageTimer
{
    gsdr_acq* a;
    hipStream_t s;
    hipEvent_t ev0{nullptr};
    StageTimer(gsdr_acq* a_, hipStream_t s_) : a(a_), s(s_) {}
    hipEvent_t take()
    {
        hipEvent_t e = nullptr;
        if (!a->prof_pool.empty())
            {
                e = a->prof_pool.back();
                a->prof_pool.pop_back();
            }
        else if (hipEventCreate(&e) != hipSuccess)
            e = nullptr;
        return e;
    }
    void begin()
    {
        if (!a->profiling) return;
        ev0 = take();
        if (ev0) (void)hipEventRecord(ev0, s);
    }
    void end(int stage)
    {
        if (!a->profiling || !ev0) return;
        hipEvent_t ev1 = take();
        if (!ev1) return;
        (void)hipEventRecord(ev1, s);
        a->prof_recs.push_back({ev0, ev1, stage});
        ev0 = nullptr;
    }
};

// acq_common.hip
AcqEnv read_acq_env();
AcqView view_of(const gsdr_acq* a);
AcqParams params_of(const gsdr_acq* a, const AcqView& v);
int rebuild_wipeoffs(gsdr_acq* a);
void compute_threshold(gsdr_acq* a);
float step_two_threshold(const gsdr_acq* a);
// argument and handle checks shared by the ABI calls; `who` names the call in the message:
// n (called `name`) in [1, max_blocks]; no bit transition, max_dwells 1 and blocks of
// fft_size items, which the modes that take each item as one grid of its own need
// (`what`: "pairs", "QuickSync")
int check_block_count(const gsdr_acq* a, const char* who, uint32_t n, const char* name);
int check_single_grid_handle(const gsdr_acq* a, const char* who, const char* what);
// bytes of device memory to the host behind the work enqueued so far on the handle's
// stream, which is synchronised
int read_back(gsdr_acq* a, void* dst_host, const void* src_dev, size_t bytes);
// the row maxima a correlate left in d_stats[p D + d] (block 0), behind the work enqueued
// so far: out[d P + p] = max / divisor (a division, as the records' normalisation is: the
// product with the reciprocal rounds differently)
int row_maxima_to_host(gsdr_acq* a, uint32_t P, uint32_t D, float divisor, float* out);
// the kernels that are no templates: rows of Doppler wipe-offs (freqs, or the main
// grid of the handle's configuration when null), the grid maximum and statistic per
// (block, PRN) or (dwells) per (block, PRN, dwell), the dwell decision, the second peak
// of gsdr_acq_run_dwell's accumulated grid
int launch_wipeoff(gsdr_acq* a, float2* wipe, uint32_t rows, const float* freqs);
// the main grid's first `rows` rows over len samples each (QuickSync's items)
int launch_wipeoff_long(gsdr_acq* a, float2* wipe, uint32_t rows, uint32_t len);
int launch_reduce(gsdr_acq* a, const AcqParams& ap, bool dwells, uint32_t nblocks, gsdr_acq_result* res,
    const uint32_t* prn, uint64_t stamp0, uint64_t stride, hipStream_t s);
int launch_decide(gsdr_acq* a, uint32_t n, gsdr_acq_result* res, hipStream_t s);
int launch_grid_second_peak(gsdr_acq* a, const AcqParams& ap, gsdr_acq_result* res, hipStream_t s);
int launch_code_lane_order(gsdr_acq* a, uint32_t first_slot, uint32_t nslots);

// acq_pk.hip
int launch_corr_variant(gsdr_acq* a, const AcqView& v, uint32_t nblocks, hipStream_t s);
int launch_argmax_variant(gsdr_acq* a, const AcqView& v, uint32_t nblocks, gsdr_acq_result* res, hipStream_t s);
int launch_forward_pk(gsdr_acq* a, const AcqView& v, const void* iq, uint32_t nblocks, uint64_t stride, hipStream_t s);
int setup_corr_variant(gsdr_acq* a, int id);
// acq_split.hip
int setup_split(gsdr_acq* a);
int launch_split(gsdr_acq* a, const AcqView& v, uint32_t nblocks, hipStream_t s);
int launch_split_argmax(gsdr_acq* a, const AcqView& v, uint32_t nblocks, gsdr_acq_result* res, hipStream_t s);
// acq_v_static.hip, acq_v_runtime.hip, acq_v_four.hip: the plans of acq_plans.h, one
// group per unit so the heavy instantiations compile in parallel
int dispatch_static(gsdr_acq* a, const AcqView& v, const AcqOp& op);
int dispatch_runtime(gsdr_acq* a, const AcqView& v, const AcqOp& op);
int dispatch_four(gsdr_acq* a, const AcqView& v, const AcqOp& op);
// acq_fine.hip: build the fine-Doppler plan and its buffers (no-op when built;
// GSDR_E_UNSUPPORTED leaves the handle as it was), free them
int fine_prepare(gsdr_acq* a);
void fine_free(gsdr_acq* a);
// acq_pair.hip: free the pair buffers
void pairs_free(gsdr_acq* a);
// acq_quicksync.hip: the wipe-off rows over an item for the grid in effect (no-op unless
// configured), free the QuickSync buffers
int quicksync_rebuild_wipeoffs(gsdr_acq* a);
void quicksync_free(gsdr_acq* a);
// acq_tong.hip: free the Tong buffers
void tong_free(gsdr_acq* a);
// acq_iqcaf.hip: free the IQ-CAF buffers
void iqcaf_free(gsdr_acq* a);
// acq.hip: the per-plan dispatch of an op, and the code spectra (with their lane-order
// copies) of slots [first_slot, first_slot + nslots) from their staged codes
int dispatch(gsdr_acq* a, const AcqView& v, const AcqOp& op);
int code_fft(gsdr_acq* a, uint32_t first_slot, uint32_t nslots);

// enqueue(iq) on items [first, first + n_items) of the ring, under one hold of the ring's
// lock from the view to the reader-event record (StreamReader); the first non-OK code.
template <class Enqueue>
int with_ring_items(gsdr_acq* a, gsdr_stream* ring, uint64_t first, uint64_t n_items, Enqueue&& enqueue)
{
    gsdr::StreamReader rd(ring);
    const void* iq = nullptr;
    int rc = rd.view(first, n_items, &iq);
    if (rc == GSDR_OK) rc = rd.acquire(a->stream);
    if (rc == GSDR_OK) rc = enqueue(iq);
    if (rc == GSDR_OK) rc = rd.release(a->stream);
    return rc;
}

}  // namespace gsdr_acq_impl
