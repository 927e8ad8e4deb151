/*
 * gsdr.h — C ABI of the MI355X-native GNSS acquisition + tracking correlator engine.
 *
 * This is the drop-in boundary for GNSS-SDR's two data-parallel hot paths:
 *
 *  - PCPS acquisition: replaces the compute of pcps_acquisition
 *    (src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.cc:176-209
 *    set_local_code, :233-305 Doppler grid, :511-612 statistics, :615-882
 *    acquisition_core, :894-909 calculate_threshold), batched over PRNs and over
 *    consecutive input blocks.
 *
 *  - Tracking multicorrelator: replaces Cpu_Multicorrelator_Real_Codes
 *    (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:37-61, .cc:36-167)
 *    and Cpu_Multicorrelator (src/algorithms/tracking/libs/cpu_multicorrelator.h:37-58),
 *    i.e. the VOLK-GNSSSDR resampler + rotator-dot-product pair, fused into one
 *    HIP launch batched over channels.
 *
 * Conventions
 *  - Every function returns int: GSDR_OK (0) or a negative GSDR_E* code.  The
 *    thread-local message of the last failure is gsdr_last_error().  No C++
 *    exception crosses this boundary.
 *  - Plain pointers and sizes only.  "host" pointers are ordinary CPU memory;
 *    "dev" pointers are HIP device memory on the handle's device; "stream" is a
 *    hipStream_t passed as void* (NULL = the handle's own stream).
 *  - Complex samples are interleaved float pairs (gr_complex / std::complex<float>),
 *    cshort samples are interleaved int16 pairs (lv_16sc_t).
 *  - A handle is owned by one caller at a time; distinct handles may be used
 *    concurrently from different threads (GNU Radio thread-per-block model).
 */
#ifndef GSDR_H
#define GSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSDR_ABI_VERSION 1

#define GSDR_OK 0
#define GSDR_E_ARG (-1)         /* invalid argument (≙ std::invalid_argument in Acq_Conf) */
#define GSDR_E_DEVICE (-2)      /* HIP runtime / device error */
#define GSDR_E_ALLOC (-3)       /* device or host allocation failed */
#define GSDR_E_STATE (-4)       /* call not valid in the handle's current state */
#define GSDR_E_UNSUPPORTED (-5) /* configuration outside what the engine implements */

/* Sample item types (Acq_Conf::item_type, acq_conf.h:42; item_type_size). */
#define GSDR_ITEM_GR_COMPLEX 0 /* complex<float>, 8 bytes */
#define GSDR_ITEM_CSHORT 1     /* complex<int16>, 4 bytes (also ishort: Ishort_To_Complex reads the same pairs) */
/* interleaved int8 I,Q, 2 bytes: SignalSource.item_type=byte through Ibyte_To_Complex
 * (data_type_adapter/adapters/ibyte_to_complex.cc:39, gr::blocks::interleaved_char_to_complex
 * with scale 1): converted exactly to complex<float> inside the kernels' loads. */
#define GSDR_ITEM_IBYTE 2

/* Float association used for the resampler code-phase index:
 * GSDR_ASSOC_GENERIC: floor((step*n + shift) - rem)   KERN/32f_xn_resampler_32f_xn.h:73
 * GSDR_ASSOC_AVX:     floor(step*n + (shift - rem))   KERN/32f_xn_resampler_32f_xn.h:384-390
 * The x86 VOLK dispatcher selects the AVX protokernel, so that is the default. */
#define GSDR_ASSOC_GENERIC 0
#define GSDR_ASSOC_AVX 1

const char* gsdr_last_error(void);
int gsdr_abi_version(void);
/* Number of HIP devices visible to this process. */
int gsdr_device_count(int* count);
/* Page-lock a host buffer (the flowgraph's sample buffer upstream of the blocks) so
 * gsdr_stream_push / the host-input calls copy it to HBM by DMA without a staging
 * copy; gsdr_host_unregister before the buffer is freed.  No reference counterpart
 * (GNU Radio buffers are pageable; gr-cuda style custom buffers would pin them). */
int gsdr_host_register(void* ptr, size_t bytes);
int gsdr_host_unregister(void* ptr);

/* ======================================================================== */
/* Device IQ ring indexed by absolute sample count                           */
/* ======================================================================== */
/*
 * The input stream uploaded once per GPU and read in place by every consumer --
 * the acquisition grid and the tracking channel pool -- by absolute sample
 * index: the nitems_read index dll_pll_veml_tracking consumes by
 * (dll_pll_veml_tracking.cc:1797,1818,2122) and the sample counter
 * pcps_acquisition stamps its results with (pcps_acquisition.cc:968,1009).  In a
 * GNU Radio flowgraph one block pushes each general_work call's items; the
 * acquisition and tracking blocks then launch on windows of the ring instead of
 * copying their own host buffers.
 *
 * capacity_items ring positions (sample % capacity) plus a mirror of the first
 * max_window_items positions, so every window of up to max_window_items items
 * is one contiguous device span.  The ring keeps the last capacity_items items.
 */
typedef struct gsdr_stream gsdr_stream;

int gsdr_stream_create(int device, int item_type, uint64_t capacity_items, uint64_t max_window_items, gsdr_stream** out);
void gsdr_stream_destroy(gsdr_stream* stream);
/* Append n items (item_type of the ring) whose first one is absolute input sample
 * first_sample; pushes are contiguous (first_sample = the previous push's end;
 * the first push sets the origin).  Asynchronous H2D on the ring's copy stream,
 * ordered after every consumer launch issued so far (no overwrite of data in
 * use); n <= capacity_items.
 * Lifetime of iq_host: the copy reads it after the call returns (from page-locked
 * memory, gsdr_host_register, it is a DMA straight from the caller's buffer), so
 * the n items must stay valid and unchanged until the push has landed:
 * gsdr_stream_landed reports *landed >= first_sample + n, or
 * gsdr_stream_wait_landed(stream, first_sample + n) returned.  A GNU Radio block
 * that pushes its input items therefore consumes (consume_each) only items that
 * landed -- the scheduler recycles consumed items upstream
 * (dll_pll_veml_tracking.cc:2119). */
int gsdr_stream_push(gsdr_stream* stream, const void* iq_host, uint64_t first_sample, uint64_t n);
/* Every item before *landed is in device memory: the host memory of the pushes that
 * ended there may be reused.  Non-blocking. */
int gsdr_stream_landed(gsdr_stream* stream, uint64_t* landed);
/* Waits until every push holding an item before `upto` has landed. */
int gsdr_stream_wait_landed(gsdr_stream* stream, uint64_t upto);
/* The longest contiguous window ending at the newest item: [*first_sample,
 * *first_sample + *n_items). */
int gsdr_stream_span(gsdr_stream* stream, uint64_t* first_sample, uint64_t* n_items);
/* Device pointer of items [first_sample, first_sample + n_items) after the pushes
 * so far have landed (synchronises with the copy stream); GSDR_E_ARG if the window
 * is not (or no longer) in the ring.  For host-synchronous readers: the pointer
 * stays valid until the next push.  A reader whose kernels run on a stream uses
 * the pair below instead. */
int gsdr_stream_window(gsdr_stream* stream, uint64_t first_sample, uint64_t n_items, const void** iq_dev);
/* Asynchronous reader: the same window, with consumer_stream (a hipStream_t)
 * made to wait for the pushes so far; after enqueuing its reads the caller calls
 * gsdr_stream_release(stream, consumer_stream), and every later push waits for
 * those reads before it overwrites ring positions.  Between the two calls the
 * window is open: a push from another thread that would overwrite it blocks
 * until the release, and such a push from the thread that opened it returns
 * GSDR_E_STATE (release first).  With pushes from another thread, the caller keeps
 * the two calls and its launches between them free of any wait on that thread.
 * The library's own consumers (gsdr_acq_run_stream, gsdr_trk_run_stream) hold the
 * ring lock from window to release. */
int gsdr_stream_window_async(gsdr_stream* stream, uint64_t first_sample, uint64_t n_items, void* consumer_stream,
    const void** iq_dev);
int gsdr_stream_release(gsdr_stream* stream, void* consumer_stream);
/* The device the ring lives on (a consumer handle must be on the same device). */
int gsdr_stream_device(const gsdr_stream* stream, int* device);
/* Synchronous device-to-host copy of items [first, first + n) of any ring (after
 * the pushes, or the decimator passes, so far): for tests and dumps.  GSDR_E_ARG
 * if the ring does not hold them (any more). */
int gsdr_stream_read(gsdr_stream* stream, uint64_t first, uint64_t n, void* host_out);

/* ======================================================================== */
/* Acquisition resampler — decimating low-pass FIR between two rings         */
/* ======================================================================== */
/*
 * GNSS-SDR.use_acquisition_resampler: the reference inserts one
 * gr::filter::fir_filter_ccf with firdes::low_pass taps per signal and RF channel
 * in front of the acquisition blocks (gnss_flowgraph.cc:1012-1128), and PCPS runs
 * at Acq_Conf::resampled_fs.  A gsdr_decim reads a source ring of any item type
 * and fills a GSDR_ITEM_GR_COMPLEX ring of its own on the same device:
 *
 *   y[m] = sum_{j=0}^{T-1} taps[j] * x[m*d - j]
 *
 * over absolute source sample indices, x = 0 before the source's first pushed
 * sample `base` (GNU Radio's zero history).  The first output is m0 =
 * ceil(base / d); output m is ready once source item m*d has been pushed.  An
 * output index times d is an input sample index (pcps_acquisition.cc:705).  fp32
 * with one summation order per output (j ascending, fused multiply-add): the
 * output bytes do not depend on how the input was split into pushes and calls.
 */
typedef struct gsdr_decim gsdr_decim;

/* firdes::low_pass with the Hamming window.  Host-only.  *ntaps: capacity of taps
 * in, tap count out (GSDR_E_ARG if the design does not fit).
 *   ntaps = (int)(53 fs / (22 transition_width)), made odd by +1; M = (ntaps-1)/2;
 *   w[n] = 0.54 - 0.46 cos(2 pi n / (ntaps-1)) as float; omega = 2 pi cutoff / fs;
 *   taps[n+M] = (n == 0 ? omega/pi : sin(n omega)/(n pi)) w[n+M] as float,
 *   scaled by gain / (taps[M] + 2 sum_{n=1..M} taps[n+M]).
 * GSDR_E_ARG unless 0 < cutoff <= fs/2 and transition_width > 0. */
int gsdr_firdes_low_pass(double gain, double fs, double cutoff, double transition_width, float* taps, uint32_t* ntaps);
/* The resampler the reference builds for an acquisition at fs_in whose signal's
 * optimum acquisition rate is opt_fs (acq_conf.cc:97-106,
 * gnss_flowgraph.cc:1073-1087,1112): decimation = floor(fs_in / opt_fs) lowered to
 * a divisor of fs_in; taps low_pass(1, fs_in, fs_d / 2.1, fs_d / 2) with fs_d =
 * fs_in / decimation; latency = (ntaps - 1) / 2 input samples.  decimation 1 with
 * ntaps = latency = 0: no resampler (fs_in <= opt_fs, or no divisor above 1). */
int gsdr_acq_resampler_plan(int64_t fs_in, double opt_fs, uint32_t* decimation, uint32_t* ntaps, uint32_t* latency);
/* 1 <= decimation <= 64 and 1 <= ntaps <= 1024 (GSDR_E_UNSUPPORTED beyond, GSDR_E_ARG
 * for 0); the source ring's window must hold ntaps + decimation items.  The output
 * ring (capacity_items, max_window_items as in gsdr_stream_create) belongs to the
 * decimator: gsdr_decim_destroy destroys it, the caller never does, and
 * gsdr_stream_push on it returns GSDR_E_STATE.  The source must outlive the
 * decimator. */
int gsdr_decim_create(gsdr_stream* source, uint32_t decimation, const float* taps, uint32_t ntaps, uint64_t capacity_items,
    uint64_t max_window_items, gsdr_decim** out);
void gsdr_decim_destroy(gsdr_decim* decim);
/* The decimated ring: every consumer of a gsdr_stream reads it unchanged. */
int gsdr_decim_output(gsdr_decim* decim, gsdr_stream** out);
/* Filters every output that became ready since the last call; *out_head (may be
 * NULL) is the output ring's head afterwards.  Asynchronous: the kernels wait for
 * the source's pushes on the device and are recorded as a reader of the source;
 * a backlog longer than the source's window takes several kernel passes.
 * GSDR_E_STATE (reason in gsdr_last_error) when the source ring no longer holds
 * the ntaps - 1 history items or the unfiltered backlog, or when a window of the
 * output ring that a pass would overwrite is still open. */
int gsdr_decim_advance(gsdr_decim* decim, uint64_t* out_head);

/* ======================================================================== */
/* Acquisition — PCPS (pcps_acquisition)                                     */
/* ======================================================================== */

typedef struct gsdr_acq gsdr_acq;

/* Mirrors the Acq_Conf fields (acq_conf.h:33-82) that drive acquisition_core. */
typedef struct gsdr_acq_conf
{
    int64_t fs_in;                /* sampling rate after optional resampling [sps]   (resampled_fs) */
    uint32_t consumed_samples;    /* samples per block = sampled_ms*samples_per_ms    (pcps_acquisition.cc:71) */
    uint32_t fft_size;            /* 0 -> derived as in pcps_acquisition.cc:85-92 */
    float samples_per_code;       /* Acq_Conf::samples_per_code */
    uint32_t samples_per_chip;    /* Acq_Conf::samples_per_chip (peak-ratio exclusion window) */
    int32_t doppler_max;          /* [Hz] */
    uint32_t doppler_step;        /* [Hz] */
    int32_t doppler_center;       /* [Hz] */
    int32_t doppler_bias;         /* [Hz] FDMA bias (is_fdma, pcps_acquisition.cc:212-230) */
    uint32_t num_doppler_bins;    /* 0 -> ceil(2*doppler_max/doppler_step)            (pcps_acquisition.cc:264) */
    float pfa;                    /* > 0: CFAR max/input-power statistic; == 0: first/second peak */
    uint32_t max_dwells;          /* non-coherent dwells per acquisition attempt (forced to 1 with bit_transition_flag) */
    int32_t bit_transition_flag;  /* consumed = 2 x sampled span, code in the second half, outputs [N/2, N) */
    int32_t item_type;            /* GSDR_ITEM_* */
    uint32_t max_prns;            /* capacity: PRNs per batch */
    uint32_t max_blocks;          /* capacity: blocks per call */
    uint32_t sampled_ms;          /* Acq_Conf::sampled_ms */
    uint32_t ms_per_code;         /* Acq_Conf::ms_per_code */
} gsdr_acq_conf;

/* One acquisition outcome per (block, PRN): the Gnss_Synchro fields written by
 * acquisition_core (pcps_acquisition.cc:697-713) plus the statistic inputs. */
typedef struct gsdr_acq_result
{
    uint32_t prn;
    uint32_t doppler_index;   /* d* */
    uint32_t code_phase;      /* indext: n* in the (effective) FFT row */
    int32_t doppler_hz;       /* Acq_doppler_hz */
    float peak;               /* grid maximum |R|^2 */
    float input_power;        /* CFAR: mean |R|^2 of row (d*+D/2)%D / 2 / dwells; 0 for peak-ratio */
    float second_peak;        /* peak-ratio: second peak outside +-1 chip; 0 for CFAR */
    float test_statistic;     /* d_test_statistics */
    double acq_delay_samples; /* Acq_delay_samples = fmod(indext, samples_per_code) */
    uint64_t samplestamp;     /* Acq_samplestamp_samples */
    int32_t positive;         /* test_statistic > threshold */
    int32_t num_dwells;       /* dwells integrated when the decision was taken (1..max_dwells) */
} gsdr_acq_result;

int gsdr_acq_create(int device, const gsdr_acq_conf* conf, gsdr_acq** out);
void gsdr_acq_destroy(gsdr_acq* acq);

/* Doppler bins D actually used, and the FFT size. */
int gsdr_acq_get_dims(const gsdr_acq* acq, uint32_t* num_doppler_bins, uint32_t* fft_size);
/* The FFT plan the handle runs on (for tests and diagnostics; no effect on the engine).
 * *variant: 1-4 compile-time LDS plans, 10-12 runtime LDS plans on 256 / 512 / 1024
 * threads, 20 / 22 the generic four-step on 256 / 1024 threads, 24-27 the packed
 * four-step.  *nthreads: the workgroup size of the variant's kernels.  *r1: the
 * four-step's register radix R (N = R * N2), 0 for an LDS size.  *nstages and radix[]:
 * the stages of the LDS plan, or of the N2 sub-plan of a four-step; *nstages = 0 for
 * the packed four-step's compile-time sub-plans; radix[i] = 1 for i >= *nstages.  Any
 * output pointer may be null. */
int gsdr_acq_get_plan(const gsdr_acq* acq, int32_t* variant, int32_t* nthreads, int32_t* r1, int32_t* nstages,
    int32_t radix[8]);
/* The split register four-step correlate in effect (0: none): 1 / 25 for 25000 with one /
 * two PRNs per workgroup (GSDR_ACQ_PPW), 4 / 24 for 100000 with one / two sub-transforms
 * per workgroup (GSDR_ACQ_QPW), 12 for 32000, 13 for 64000; GSDR_ACQ_SPLIT=0 and
 * max_dwells > 1 give 0. */
int gsdr_acq_get_split(const gsdr_acq* acq, int32_t* split);

/* set_local_code for a batch of PRNs (pcps_acquisition.cc:176-209): codes is
 * nprn rows of consumed_samples complex<float> (host); the engine places each in
 * the FFT buffer, transforms and conjugates on the device.  prn[] are the PRN ids
 * reported back in gsdr_acq_result. */
int gsdr_acq_set_local_codes(gsdr_acq* acq, const float* codes, const uint32_t* prn, uint32_t nprn);
/* set_local_code of one PRN slot (pcps_acquisition.cc:176-209, called once per PRN
 * assignment by the channel, gps_l1_ca_pcps_acquisition.cc:151-170): code is
 * consumed_samples complex<float> (host), transformed into slot `slot` of the
 * handle's code spectra; the other slots keep theirs.  Extends the active PRN
 * count to slot + 1 if needed.  Ordered after the launches already issued. */
int gsdr_acq_set_local_code(gsdr_acq* acq, uint32_t slot, const float* code, uint32_t prn);
/* Number of PRN slots [0, nprn) the grid launches search (each with a spectrum set
 * by gsdr_acq_set_local_code[s]). */
int gsdr_acq_set_active_prns(gsdr_acq* acq, uint32_t nprn);

/* Doppler setters (AcquisitionInterface, acquisition_interface.h:56-59).  They
 * rebuild the Doppler wipe-off grid on the device, re-derive the forward-spectrum
 * reuse (gsdr_acq_get_spectrum_reuse) and, with pfa > 0, recompute the threshold;
 * the code spectra and the second step's settings stay.  The handle's buffers are
 * sized by its number of Doppler bins: a call that would change
 * ceil(2 doppler_max / doppler_step) is GSDR_E_UNSUPPORTED and doppler_step = 0 is
 * GSDR_E_ARG, both leaving the handle as it was.  A handle created with an explicit
 * num_doppler_bins keeps that count whatever the new maximum and step: its rows
 * become -doppler_max + doppler_center + doppler_step * d, d < num_doppler_bins,
 * exactly as if it had been created with the new values. */
int gsdr_acq_set_doppler(gsdr_acq* acq, int32_t doppler_max, uint32_t doppler_step, int32_t doppler_center);

/* Carrier wipe-off model of the Doppler grid (update_local_carrier,
 * pcps_acquisition.cc:233-246, through volk_gnsssdr_s32f_sincos_32fc):
 *   GSDR_WIPE_EXACT   exp(-j 2 pi f n / fs), phase reduced and evaluated in fp64,
 *                     rounded once (default);
 *   GSDR_WIPE_GENERIC the generic protokernel bit for bit (KERN/s32f_sincos_32fc.h:390-403:
 *                     one fp32 phase accumulator, cosf / sinf);
 *   GSDR_WIPE_AVX2    the a_avx2 protokernel the reference dispatches on AVX2 x86-64
 *                     (:448-627: eight fp32 accumulators, Cephes polynomials).
 * The protokernels' fp32 phase accumulators drift from the exact carrier (GPS 4 Msps:
 * 1e-3 / 2e-5 rad over 1 ms; Galileo 8 Msps, 8 ms: 0.15 / 0.01 rad); DESIGN.md 3.
 * With EXACT and Doppler bins commensurate with the FFT bins (doppler_step * N / fs =
 * p / q, q <= D / 2) the forward pass computes q spectra per block and every Doppler
 * row is an exact circular shift of one of them (gsdr_acq_get_spectrum_reuse).
 * Initial mode: GSDR_ACQ_WIPE=exact|generic|avx2 in the environment, else EXACT. */
#define GSDR_WIPE_EXACT 0
#define GSDR_WIPE_GENERIC 1
#define GSDR_WIPE_AVX2 2
int gsdr_acq_set_wipeoff(gsdr_acq* acq, int mode);
/* The forward-spectrum reuse in effect: *q spectra per block (== D: none), each
 * Doppler class step shifting by *p bins. */
int gsdr_acq_get_spectrum_reuse(const gsdr_acq* acq, uint32_t* q, uint32_t* p);

/* Threshold: set explicitly (set_threshold) or computed from pfa exactly as
 * calculate_threshold (pcps_acquisition.cc:894-909). */
int gsdr_acq_set_threshold(gsdr_acq* acq, float threshold);
int gsdr_acq_get_threshold(const gsdr_acq* acq, float* threshold);

/* Synchronous drop-in: nblocks acquisition attempts over consecutive blocks of
 * consumed_samples items (item_type) from host memory.  Attempt i integrates up
 * to max_dwells blocks (block j = i*max_dwells + k for dwell k, sample stamp
 * stamp0 + j*consumed) and reports, per PRN, the first dwell whose statistic
 * crosses the threshold or else the last (acquisition_core's dwell loop,
 * pcps_acquisition.cc:781-869); with max_dwells = 1 an attempt is one block.
 * out: nblocks*nprn results, attempt-major (host). */
int gsdr_acq_run(gsdr_acq* acq, const void* iq_host, uint32_t nblocks, uint64_t stamp0, gsdr_acq_result* out);

/* acquisition_core's dwell loop one block per call, as the reference block runs
 * it (pcps_acquisition.cc:637-680, :781-829): dwell = the call's
 * d_num_noncoherent_integrations_counter - 1 (0 <= dwell < max_dwells).  Dwell 0
 * starts a device-resident |R|^2 grid per PRN, later dwells add this block's
 * |R|^2 into it (volk_32f_x2_add_32f); the statistic is evaluated on the
 * accumulated grid with the counter as the CFAR divisor (:534), against the
 * max_dwells threshold (:908).  iq_host: one block (consumed_samples items);
 * out: nprn results (num_dwells = dwell + 1).  Synchronous.  The caller keeps
 * the dwell FSM (positive / next dwell / negative after max_dwells).
 * Dwell 0 restarts the grid wherever the previous attempt stopped, so an
 * abandoned attempt needs no reset.  No other call on the handle touches the
 * kept grid (gsdr_acq_run and the spectrum / grid dumps between two dwells
 * leave the later dwells unchanged).  The grid is kept per PRN slot: change the
 * active PRN count (gsdr_acq_set_active_prns) between attempts, not inside one.
 * Valid on every handle, max_dwells = 1 and bit_transition_flag (which forces
 * max_dwells to 1) included: dwell >= max_dwells is GSDR_E_ARG. */
int gsdr_acq_run_dwell(gsdr_acq* acq, const void* iq_host, uint32_t dwell, uint64_t stamp, gsdr_acq_result* out);

/* Device-resident form: iq_dev holds nblocks*max_dwells blocks, block j starting
 * at item j*block_stride_items.  Results are written to out_dev (device memory,
 * nblocks*nprn).  Asynchronous on stream; no host synchronisation. */
int gsdr_acq_run_device(gsdr_acq* acq, const void* iq_dev, uint32_t nblocks, uint64_t block_stride_items,
    uint64_t stamp0, gsdr_acq_result* out_dev, void* stream);

/* Ring form: nblocks attempts on the ring's items from absolute sample
 * first_sample on (the nblocks*max_dwells consecutive blocks gsdr_acq_run would
 * read from a contiguous host buffer), results to out_host (nblocks*nprn), sample
 * stamps from stamp0 as in gsdr_acq_run.  The launch waits for the ring's
 * pushes on the device (no host synchronisation before it) and is ordered before
 * later pushes overwrite the window.  Synchronous (results on the host). */
int gsdr_acq_run_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nblocks, uint64_t stamp0,
    gsdr_acq_result* out_host);
/* Asynchronous ring form (the batched acquisition service's call, gnss_flowgraph.cc:
 * 1796-1901 answered per block): the grids of nblocks attempts from first_sample are
 * launched on the handle's stream with the results copied into the handle's pinned
 * buffer; returns without waiting.  gsdr_acq_collect waits for them and copies the
 * nblocks * nprn results (block-major, nprn = the active count at submission) to
 * out_host.  Up to two submissions in flight per handle (the second queued behind
 * the first on the handle's stream), collected oldest first. */
int gsdr_acq_submit_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nblocks,
    uint64_t stamp0);
int gsdr_acq_collect(gsdr_acq* acq, gsdr_acq_result* out_host, uint32_t* nblocks, uint32_t* nprn);

/* The reference's acquisition grid dump (pcps_acquisition.cc:408-508): writes the
 * |R|^2 grid of PRN slot `prn_slot` for one host block into grid_host
 * (D rows of fft_size floats, Doppler-major).  Synchronous. */
int gsdr_acq_dump_grid(gsdr_acq* acq, const void* iq_host, uint32_t prn_slot, float* grid_host);
/* The correlate pass's own product for one host block: the forward spectra, then the
 * handle's packed correlate variant (the kernel a run launches, on the active PRN
 * slots), then its row maxima max_n |R_{d,p}[n]|^2 into out_host, D rows of nprn
 * floats (Doppler-major).  A run shows these only through the Doppler row that wins;
 * gsdr_acq_dump_grid recomputes the rows with another kernel.  GSDR_E_UNSUPPORTED for
 * a handle without a packed variant (other FFT sizes, dwells, bit transition).
 * Synchronous. */
int gsdr_acq_dump_row_maxima(gsdr_acq* acq, const void* iq_host, float* out_host);
/* The narrow grid of make_two_steps for the same dump (d_narrow_grid,
 * pcps_acquisition.cc:743-746, written by dump_results :493-506): the |R|^2 grid of
 * PRN slot prn_slot over the num_doppler_bins_step2 rows centred on
 * doppler_center_hz (update_grid_doppler_wipeoffs_step2, :307-314) for one host
 * block, into grid_host (num_doppler_bins_step2 rows of fft_size floats).  Needs
 * gsdr_acq_set_step_two and num_doppler_bins_step2 <= the handle's Doppler bins.
 * Synchronous. */
int gsdr_acq_dump_grid_step_two(gsdr_acq* acq, const void* iq_host, uint32_t prn_slot, float doppler_center_hz,
    float* grid_host);

/* make_two_steps (pcps_acquisition.cc:298-314, :717-773, :781-800, :894-909;
 * Acq_Conf second_nbins / second_doppler_step / pfa_second_step, acq_conf.cc:63-76).
 * After a positive first step the reference searches the NEXT block on a narrow
 * grid of num_doppler_bins_step2 bins spaced doppler_step2 Hz around the coarse
 * Acq_doppler_hz (float arithmetic, no doppler_bias), with its own threshold
 * (pfa2 and the narrow bin count; pfa2 outside (0,1] means pfa as in Acq_Conf)
 * and, for CFAR, the first step's input power (d_input_power is not recomputed
 * in step two, :530-540).  set_step_two configures the narrow grid for the
 * handle; run_step_two runs it for nsel PRN slots of the current batch over one
 * attempt (max_dwells blocks) of host IQ, prn_slots[i] with centre
 * doppler_center_hz[i] (the coarse Acq_doppler_hz) and coarse_input_power[i]
 * (the coarse result's input_power; ignored by the peak-ratio statistic).
 * out[i]: the step-two Gnss_Synchro fields (doppler_hz from the narrow grid,
 * :539) and the decision against the step-two threshold.  Synchronous. */
int gsdr_acq_set_step_two(gsdr_acq* acq, uint32_t num_doppler_bins_step2, float doppler_step2, float pfa2);
int gsdr_acq_get_step_two_threshold(const gsdr_acq* acq, float* threshold);
int gsdr_acq_run_step_two(gsdr_acq* acq, const void* iq_host, uint32_t nsel, const uint32_t* prn_slots,
    const float* doppler_center_hz, const float* coarse_input_power, uint64_t stamp, gsdr_acq_result* out);

/* Stage profiling with HIP events recorded on the launch stream (observability,
 * the role of the reference's per-block timing prints).  When enabled, every
 * gsdr_acq_run / gsdr_acq_run_device call records device time per stage:
 * [0] forward FFT (x .* w_d), [1] fused correlate (code product + inverse FFT +
 * |.|^2 + row statistics), [2] grid reduction, [3] second-peak pass.
 * gsdr_acq_read_profile synchronises, returns the sums since the last read
 * (milliseconds) and the number of launches per stage, and resets them. */
int gsdr_acq_set_profiling(gsdr_acq* acq, int enable);
int gsdr_acq_read_profile(gsdr_acq* acq, double* stage_ms, uint32_t* launches);
/* The same, plus per stage the busy time: the union of its launches' [start, end)
 * intervals (stage_busy_ms may be NULL) -- the stage's wall time when launches of
 * the handle overlap (runs issued on several streams); stage_ms / launches then
 * over-counts it. */
int gsdr_acq_read_profile_ex(gsdr_acq* acq, double* stage_ms, uint32_t* launches, double* stage_busy_ms);
/* The recorded launches of one stage (0 forward, 1 correlate, 2 reduce/argmax,
 * 3 second peak) as [start, end) in ms against the caller's hipEvent_t ref_event
 * (recorded on the same device before them), so the busy time of one stage over
 * several handles -- chains on their own streams -- is the union of all their
 * intervals.  *n = the stage's launch count (entries beyond max_n not written).
 * Read before gsdr_acq_read_profile[_ex], which releases the records. */
int gsdr_acq_read_profile_intervals(gsdr_acq* acq, const void* ref_event, int stage, double* start_ms, double* end_ms,
    uint32_t max_n, uint32_t* n);

/* Debug/verification: device forward spectrum for one host block,
 * D rows x fft_size complex<float> (= FFT(x .* w_d)). */
int gsdr_acq_dump_spectra(gsdr_acq* acq, const void* iq_host, float* spectra_host);

/* ---- Fine Doppler: the second stage of pcps_acquisition_fine_doppler_cc
 * (estimate_Doppler, pcps_acquisition_fine_doppler_cc.cc:346-419).  With N = fft_size,
 * the block wipes the code off 10 ms of signal (L = 10 N samples) with the replica
 * aligned to the coarse code phase, zero-pads to M = 8 L = 80 N points, takes one
 * M-point FFT and the first maximum of |X|^2: a Doppler on a grid of fs / (80 N) Hz,
 * accepted if within 1000 Hz of the coarse one.  The engine computes the padded
 * transform as eight L-point transforms of the wiped signal times a phase ramp, one
 * workgroup per (request, residue of the bin index mod 8), and never stores the
 * spectrum.  The replica alignment is the reference's, quirk included (:365-371):
 * std::rotate(c, c + (N - shift), c + N - 1) ends its range at N - 1, so only the
 * first N - 1 samples rotate, sample N - 1 stays, and shift 0 and 1 both leave the row
 * unchanged; the ten periods are copies of that row (:373-376).
 * Only handles on 1 ms blocks (consumed_samples == fft_size, no bit_transition_flag)
 * and sizes whose L has an FFT plan (2^a 3^b 5^c; up to 20352 points in LDS, else
 * R x N2 with R in {8, 10, 12, 16, 20, 25}) are served: GSDR_E_UNSUPPORTED otherwise,
 * the handle unchanged.  The plan, its tables and its scratch rows (a pool of 32 rows of L
 * complex, 64 from the first call with more than four requests on) are built on the
 * first call (at create with GSDR_ACQ_FINE=1 in the environment) and freed with the
 * handle.  The calls leave the coarse stage's state alone (a call between two
 * gsdr_acq_run_dwell dwells does not change the later dwell). */
typedef struct gsdr_acq_fine_request
{
    uint32_t code_phase;      /* Acq_delay_samples of the coarse step, < fft_size (shift_index, :365) */
    float coarse_doppler_hz;  /* Acq_doppler_hz of the coarse step (:407) */
    uint32_t code_slot;       /* which of the call's code rows */
} gsdr_acq_fine_request;

typedef struct gsdr_acq_fine_result
{
    uint32_t index;     /* argmax of |X|^2 over the 80 N bins, first maximum (:385-388) */
    float peak;         /* |X|^2 there */
    float freq_hz;      /* fftFreqBins[index] (:394-404): float operands, formed in double, rounded once */
    double doppler_hz;  /* freq_hz if accepted, else coarse_doppler_hz (:407-416) */
    int32_t accepted;   /* std::abs(freq_hz - coarse_doppler_hz) < 1000 */
    int32_t pad;
} gsdr_acq_fine_result;

/* estimate_Doppler (:346-419) for nreq requests on one 10 ms window in one launch.
 * iq_host: 10 * fft_size items (item_type); codes: ncodes rows of fft_size
 * complex<float>, each the replica set_local_code gets
 * (gps_l1_ca_code_gen_complex_sampled, :363); out: nreq records.  Null pointers,
 * nreq = 0, code_phase >= fft_size and code_slot >= ncodes are GSDR_E_ARG.
 * Synchronous.  With gsdr_acq_set_profiling enabled the transform kernel is recorded
 * as stage [0] and the finish kernel as stage [2]. */
int gsdr_acq_fine_doppler(gsdr_acq* acq, const void* iq_host, const float* codes, uint32_t ncodes,
    const gsdr_acq_fine_request* requests, uint32_t nreq, gsdr_acq_fine_result* out);
/* The same on the ring's items [first_sample, first_sample + 10 * fft_size), read in
 * place (the d_10_ms_buffer copy of :494, :518-538 is not made); ordered against the
 * ring's pushes as gsdr_acq_run_stream is.  Synchronous (results on the host). */
int gsdr_acq_fine_doppler_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, const float* codes,
    uint32_t ncodes, const gsdr_acq_fine_request* requests, uint32_t nreq, gsdr_acq_fine_result* out_host);
/* Debug/verification, as gsdr_acq_dump_grid is for the coarse grid: p_tmp_vector of
 * :384-385, the |X|^2 of all 80 * fft_size bins for one code row and code phase,
 * written by the same kernels with a storing functor.  Synchronous. */
int gsdr_acq_dump_fine_spectrum(gsdr_acq* acq, const void* iq_host, const float* code, uint32_t code_phase,
    float* spectrum_host);
/* The engine of the handle's fine transform (replaces the FFTW plan of :355): *L = 10 *
 * fft_size; *r1 = 0 and *n2 = L for one LDS plan, else the four-step L = r1 * n2.  Host
 * only; any output pointer may be null; GSDR_E_UNSUPPORTED as above. */
int gsdr_acq_get_fine_plan(const gsdr_acq* acq, uint32_t* L, int32_t* r1, uint32_t* n2);
/* *ready = 1 once the handle holds its fine plan, tables and scratch pool: after the first
 * fine-Doppler call, or from create on with GSDR_ACQ_FINE=1 (and a size that has a plan). */
int gsdr_acq_get_fine_ready(gsdr_acq* acq, int32_t* ready);

/* ---- Paired-code acquisition: pcps_cccwsr_acquisition_cc (Galileo E1 CCCWSR) and
 * galileo_pcps_8ms_acquisition_cc (8 ms PCPS).  Both correlate every Doppler row with
 * two replicas per satellite; the row's value is the larger of the two row maxima ('>=':
 * the first member keeps a tie, pcps_cccwsr_acquisition_cc.cc:322), the answer the
 * first row, scanning upwards with strict '<' (:334), that holds the grid maximum, and
 * mag / input_power the statistic (:360).  Pair q occupies the handle's ordinary code
 * slots 2 q (member 0) and 2 q + 1 (member 1), so the forward and correlate kernels are
 * the plain search's.  Only handles on blocks of fft_size items (consumed_samples ==
 * fft_size), with max_dwells 1 and no bit_transition_flag are served:
 * GSDR_E_UNSUPPORTED otherwise, the handle unchanged.  Neither reference block
 * accumulates its grid over dwells: each block of a call is a grid of its own, and the
 * dwell rule over the blocks' records is the caller's. */
#define GSDR_ACQ_PAIR_AS_IS 0      /* members first[q], second[q]: the 8 ms block's code A and code B */
#define GSDR_ACQ_PAIR_SUM_DIFF_J 1 /* members first - j second, first + j second: CCCWSR's
                                    * d_correlation_plus = data + j pilot and d_correlation_minus
                                    * (:301-308) are the correlations with these two replicas */

typedef struct gsdr_acq_pair_result
{
    uint32_t prn;
    uint32_t doppler_index;   /* first row holding the grid maximum */
    uint32_t code_phase;      /* indext, < fft_size */
    uint32_t member;          /* 0 or 1: which replica holds it */
    int32_t doppler_hz;       /* Acq_doppler_hz */
    int32_t pad;
    float mag;                /* d_mag: the maximum / (float(N) float(N))^2, in float (:247, :316) */
    float input_power;        /* d_input_power: sum |x|^2 / fft_size of the block (:250-252) */
    float test_statistic;     /* mag / input_power (:360) */
    float pad2;
    double acq_delay_samples; /* code_phase % (uint32_t)samples_per_code (:337) */
    uint64_t samplestamp;     /* the block's first sample: stamp0 + b * consumed_samples */
} gsdr_acq_pair_result;

/* The replicas of npairs satellites: first and second are npairs rows of fft_size
 * complex<float>, prn their ids (CCCWSR: set_local_code(code_data, code_pilot), :126-144,
 * with GSDR_ACQ_PAIR_SUM_DIFF_J).  The members are formed on the device and transformed as
 * gsdr_acq_set_local_codes transforms its rows; the active slot count becomes 2 npairs and
 * the handle holds pairs until gsdr_acq_set_local_codes, gsdr_acq_set_local_code or
 * gsdr_acq_set_active_prns is called.  Null pointers, an unknown kind, npairs = 0 and
 * 2 npairs > max_prns are GSDR_E_ARG. */
int gsdr_acq_set_code_pairs(gsdr_acq* acq, int kind, const float* first, const float* second, const uint32_t* prn,
    uint32_t npairs);
/* nblocks independent grids over the pairs: iq_host holds nblocks * fft_size items, out
 * [nblocks][npairs] records.  The winner is the first cell in the order (row ascending,
 * member 0 before member 1, index ascending) that holds the maximum.  Synchronous.
 * GSDR_E_STATE on a handle that holds no pairs.  With gsdr_acq_set_profiling enabled the
 * input-power and merge kernels are recorded in stage [2]. */
int gsdr_acq_run_pairs(gsdr_acq* acq, const void* iq_host, uint32_t nblocks, uint64_t stamp0,
    gsdr_acq_pair_result* out);
/* The same on the ring's items from first_sample, read in place; ordered against the
 * ring's pushes as gsdr_acq_run_stream is.  Synchronous (results on the host). */
int gsdr_acq_run_pairs_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nblocks,
    uint64_t stamp0, gsdr_acq_pair_result* out_host);
/* Debug/verification: magt_plus and magt_minus (:316-320) of every Doppler row of one
 * block, out [num_doppler_bins][npairs][2] normalised row maxima, on every FFT plan. */
int gsdr_acq_dump_pair_rows(gsdr_acq* acq, const void* iq_host, float* out);

/* ---- QuickSync acquisition: pcps_quicksync_acquisition_cc.  With folding factor p and spc
 * samples per code, an item is L = p spc samples.  Every Doppler row multiplies the whole
 * item by the row's wipe-off of L samples, folds the product into Nf = spc / p points (the
 * sum of its p^2 segments, :336-343), and correlates the fold with the code folded the same
 * way (the sum of its p segments, :146-151) on an Nf-point transform.  The answer of the grid
 * is the first row, scanning upwards with strict '<' (:370), that holds the grid maximum and
 * the first index in it; the p delays index + i Nf it stands for are then told apart by p
 * correlations in time over spc samples of the wiped-off item with the unfolded code, not
 * conjugated (:383-412): the first maximum of their |.|^2 names the delay.  The handle is an
 * ordinary one created with consumed_samples == fft_size == Nf, max_dwells 1 and no
 * bit_transition_flag; the grid runs on its forward, correlate and reduce kernels, whatever
 * its pfa.  Every item of a call is a grid of its own (the block zeroes d_mag, d_input_power
 * and d_test_statistics in every state-1 call, :288-291); the dwell rule over the items'
 * records is the caller's. */
typedef struct gsdr_acq_quicksync_result
{
    uint32_t prn;
    uint32_t doppler_index;   /* first row holding the grid maximum */
    uint32_t folded_phase;    /* indext, < Nf */
    uint32_t candidate;       /* i: the delay is folded_phase + i Nf */
    int32_t doppler_hz;       /* Acq_doppler_hz */
    int32_t pad;
    float mag;                /* d_mag: the maximum / (float(Nf) float(Nf))^2, in float (:286, :367) */
    float input_power;        /* d_input_power: sum |x|^2 / L of the item (:310-312) */
    float test_statistic;     /* mag / input_power (:421) */
    float candidate_power;    /* |acc_i|^2 of the winning delay, as summed (:411) */
    double acq_delay_samples; /* folded_phase + candidate Nf (:415) */
    uint64_t samplestamp;     /* the item's first sample: stamp0 + b L */
} gsdr_acq_quicksync_result;

/* Makes the handle a QuickSync one for folding factor p and samples_per_code spc, and
 * allocates what the runs need (items of p spc samples for max_blocks items, the wipe-off
 * rows over an item, max_prns unfolded codes).  GSDR_E_ARG unless 2 <= p <= 16, spc % p == 0
 * and spc / p == the handle's fft_size.  GSDR_E_UNSUPPORTED for a handle with max_dwells > 1,
 * bit_transition_flag or consumed_samples != fft_size, and for an fft_size served by the
 * four-step plans (the fold needs a transform of one launch).  An error leaves the handle as
 * it was; plain runs on the handle are unaffected by a success too. */
int gsdr_acq_set_quicksync(gsdr_acq* acq, uint32_t folding_factor, uint32_t samples_per_code);
/* nprn unfolded replicas of samples_per_code complex<float> each, prn their ids: kept for the
 * candidate check, folded into code slots 0..nprn-1 and transformed as
 * gsdr_acq_set_local_codes transforms its rows.  The handle holds QuickSync codes until
 * gsdr_acq_set_local_codes, gsdr_acq_set_local_code, gsdr_acq_set_active_prns or
 * gsdr_acq_set_code_pairs is called.  GSDR_E_STATE before gsdr_acq_set_quicksync. */
int gsdr_acq_set_quicksync_codes(gsdr_acq* acq, const float* codes, const uint32_t* prn, uint32_t nprn);
/* nitems items of p spc host samples of the handle's item type, out [nitems][nprn] records.
 * Synchronous.  GSDR_E_STATE before both set calls; GSDR_E_UNSUPPORTED while the handle's
 * carrier model is not GSDR_WIPE_EXACT; nitems outside [1, max_blocks] is GSDR_E_ARG.  With
 * gsdr_acq_set_profiling enabled the input-power and candidate kernels are recorded in
 * stage [2]. */
int gsdr_acq_run_quicksync(gsdr_acq* acq, const void* iq_host, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_quicksync_result* out);
/* The same on the ring's samples from first_sample, read in place. */
int gsdr_acq_run_quicksync_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nitems,
    uint64_t stamp0, gsdr_acq_quicksync_result* out_host);
/* Debug/verification, one item: rows_out [num_doppler_bins][nprn] the normalised row maxima
 * (magt of every row, :367), cand_out [nprn][p] the |acc_i|^2 of the winner's p delays.
 * Either output may be null. */
int gsdr_acq_dump_quicksync(gsdr_acq* acq, const void* iq_host, float* rows_out, float* cand_out);

/* ---- Tong acquisition: pcps_tong_acquisition_cc, the variable-dwell detector.  An item is
 * N = fft_size samples.  Every item adds its |IFFT(FFT(x w_d) C)|^2 rows, scaled by
 * 1 / (fn fn P) with fn = float(N) float(N) and P the item's own input power (:268, :283-285,
 * :312-314), into a grid that lives for a whole sequence of items (:317); the statistic of an
 * item is the maximum of the accumulated grid, taken by the first row, scanning upwards with
 * strict '<' (:325), that holds it and the first index in that row (:320).  The Tong counter
 * starts at tong_init_val, goes up when the statistic exceeds threshold * dwell_count and down
 * otherwise, and ends the sequence positive at tong_max_val, negative at 0 and, whatever it
 * said, negative once dwell_count reaches tong_max_dwells (:349-372).  The handle is an
 * ordinary one created with consumed_samples == fft_size, max_dwells 1 and no
 * bit_transition_flag; its num_doppler_bins must be set to the reference's row count,
 * 2 doppler_max / doppler_step + 1 (:166-184).  Every active code slot runs a sequence of its
 * own; the threshold is gsdr_acq_set_threshold's. */
typedef struct gsdr_acq_tong_result
{
    uint32_t prn;
    uint32_t doppler_index;   /* first row holding the accumulated grid's maximum */
    uint32_t indext;          /* first index of the maximum in that row (:320) */
    int32_t doppler_hz;       /* Acq_doppler_hz */
    double acq_delay_samples; /* indext % samples_per_code (:328) */
    uint64_t samplestamp;     /* the item's first sample: stamp0 + k N (the block adds N, :272) */
    float mag;                /* d_mag = d_test_statistics: the accumulated grid's maximum */
    float input_power;        /* d_input_power: sum |x|^2 / N of the item */
    uint32_t dwell_count;     /* d_dwell_count after the item */
    uint32_t tong_count;      /* d_tong_count after the item */
    uint32_t state;           /* GSDR_TONG_* */
    uint32_t pad;             /* 0 */
} gsdr_acq_tong_result;

#define GSDR_TONG_RUNNING 0  /* the sequence goes on */
#define GSDR_TONG_POSITIVE 1 /* the item ended it: positive acquisition (state 2 of the block) */
#define GSDR_TONG_NEGATIVE 2 /* the item ended it: negative acquisition (state 3 of the block) */
#define GSDR_TONG_PAST_END 3 /* the item lies after the sequence's end and is no part of it: only prn,
                              * samplestamp, input_power and the final counts are set */

/* Makes the handle a Tong one and allocates the grid (max_prns x num_doppler_bins x fft_size
 * floats), the slots' sequence state and the per-item scales and row maxima of max_blocks
 * items; every slot starts as gsdr_acq_tong_reset leaves it.  GSDR_E_ARG unless
 * 1 <= tong_init_val < tong_max_val and tong_max_dwells >= 1 (the reference's unsigned counter
 * wraps from init 0, and init >= max never meets its '==').  GSDR_E_UNSUPPORTED for a handle
 * with max_dwells > 1, bit_transition_flag or consumed_samples != fft_size, for an fft_size
 * served by the four-step plans and while the carrier model is not GSDR_WIPE_EXACT.  An error
 * leaves the handle as it was; plain runs on the handle are unaffected by a success too.  The
 * codes are those of gsdr_acq_set_local_codes. */
int gsdr_acq_set_tong(gsdr_acq* acq, uint32_t tong_init_val, uint32_t tong_max_val, uint32_t tong_max_dwells);
/* set_state(1) for nslots code slots (slots null: all of them): counts back to their start,
 * sequence running, and the slot's next item starts its rows from zero.  A slot >= max_prns is
 * GSDR_E_ARG; GSDR_E_STATE before gsdr_acq_set_tong. */
int gsdr_acq_tong_reset(gsdr_acq* acq, const uint32_t* slots, uint32_t nslots);
/* nitems consecutive host items of fft_size samples of the handle's item type, continuing
 * every slot's sequence from where the previous call left it; out [nitems][nprn] records.
 * Items past a sequence's end, in this call or a later one, are GSDR_TONG_PAST_END until the
 * slot is reset.  Synchronous, one stream synchronisation per call.  GSDR_E_STATE before
 * gsdr_acq_set_tong or without plain codes; GSDR_E_UNSUPPORTED while the carrier model is not
 * GSDR_WIPE_EXACT; nitems outside [1, max_blocks] is GSDR_E_ARG.  With gsdr_acq_set_profiling
 * enabled the forward pass is recorded in stage [0], the grid kernel in [1] and the input
 * powers and the counter kernel in [2]. */
int gsdr_acq_run_tong(gsdr_acq* acq, const void* iq_host, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_tong_result* out);
/* The same on the ring's samples from first_sample, read in place. */
int gsdr_acq_run_tong_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nitems,
    uint64_t stamp0, gsdr_acq_tong_result* out_host);
/* Debug/verification: the accumulated grid of a slot as it stands, [num_doppler_bins][fft_size]
 * floats.  Rows of a slot that has seen no item since its reset are reported as zeros. */
int gsdr_acq_dump_tong_grid(gsdr_acq* acq, uint32_t prn_slot, float* grid_host);

/* ---- E5a non-coherent IQ acquisition with CAF filter:
 * galileo_e5a_noncoherent_iq_acquisition_caf_cc.  An item is N = fft_size samples.  Every Doppler
 * row correlates the data replica (I) and, with both components, the pilot replica (Q); with 2 or
 * 3 ms of coherent integration also the B form of each, the replica with its first code period
 * negated (:186-205).  Per component the form with the larger normalised peak is chosen ('>=': A
 * keeps a tie, :455, :464) -- the reference reads the Q-B peak from the I-B row (:445), which is
 * kept -- and the two chosen |.|^2 rows are added cell by cell; the maximum of the sum is the
 * row's value (:470-546).  The answer of the grid is the first row, scanning upwards with strict
 * '<' (:549), that holds the maximum.  With caf_window_hz > 0 the chosen components' raw peaks
 * over the rows pass the weighted window of :599-668, whose first maximum names the Doppler the
 * block reports (:670-672).  The handle is an ordinary one created with consumed_samples ==
 * fft_size, max_dwells 1 and no bit_transition_flag; its num_doppler_bins must be set to the
 * reference's row count, 2 doppler_max / doppler_step + 1 (:227-232).  Every item of a call is a
 * grid of its own; the dwell rule over the items' records (:549-568, :686-700) is the caller's. */
typedef struct gsdr_acq_iq_caf_row
{
    uint32_t choice_i;        /* 0: the I-A row was chosen, 1: I-B (:455) */
    uint32_t choice_q;        /* 0: Q-A, 1: Q-B (:464); 0 with one component */
    float peak_i;             /* d_CAF_vector_I: the chosen I row's own raw maximum */
    float peak_q;             /* d_CAF_vector_Q: the chosen Q row's own raw maximum (Q-B's true one); 0 with one component */
    float sum_peak;           /* raw maximum of the summed row (of the chosen I row with one component) */
    uint32_t sum_index;       /* its first index */
} gsdr_acq_iq_caf_row;

typedef struct gsdr_acq_iq_caf_result
{
    uint32_t prn;
    uint32_t doppler_index;     /* first row holding the grid maximum (:549) */
    uint32_t caf_doppler_index; /* first maximum of d_CAF_vector (:670); == doppler_index with the filter off */
    uint32_t indext;            /* first index of the maximum in the winning row's sum */
    int32_t doppler_hz;         /* the grid winner's Doppler (:562) */
    int32_t caf_doppler_hz;     /* the filter's Doppler (:671); == doppler_hz with the filter off */
    float mag;                  /* d_mag: the maximum / (fn fn), fn = float(N) float(N), in float (:373, :488) */
    float input_power;          /* d_input_power: sum |x|^2 / N of the item (:385-387) */
    float test_statistic;       /* mag / input_power (:566) */
    float pad;                  /* 0 */
    double acq_delay_samples;   /* indext % samples_per_code (:561) */
    uint64_t samplestamp;       /* the item's first sample: stamp0 + k N */
} gsdr_acq_iq_caf_result;

/* Makes the handle an IQ-CAF one and allocates what the runs need (the caller's replica rows,
 * the rows' records and the results of max_blocks items, and the |.|^2 rows of a workgroup
 * where they do not fit its LDS).  coherent_ms is 1 to 3 (1 also for the zero-padded form: the
 * block then holds only the A forms, :104-107); a satellite takes 1, 2 or 4 code slots (I-A, I-B
 * when coherent_ms > 1, Q-A when both_components, Q-B when both hold), and max_prns bounds slots
 * x satellites.  GSDR_E_ARG for samples_per_code 0 or > fft_size, coherent_ms outside [1,3], and
 * where the reference would divide by zero or index outside its vectors: caf_window_hz > 0 with
 * caf_window_hz / (2 doppler_step) == 0 or with 2 (caf_window_hz / (2 doppler_step)) + 1 >
 * num_doppler_bins.  GSDR_E_UNSUPPORTED for a handle with max_dwells > 1, bit_transition_flag or
 * consumed_samples != fft_size and while the carrier model is not GSDR_WIPE_EXACT.  Every FFT plan
 * is served.  GSDR_ACQ_IQCAF_ROWS_HBM=1 (read at create) keeps the workgroup's rows in device
 * memory at every size.  An error leaves the handle as it was. */
int gsdr_acq_set_iq_caf(gsdr_acq* acq, uint32_t samples_per_code, uint32_t coherent_ms, int both_components,
    int32_t caf_window_hz);
/* The replicas of nsat satellites as the adapter hands them to set_local_code (:160): code_i and
 * code_q are nsat rows of fft_size complex<float>, already tiled coherent_ms times or zero padded;
 * code_q is null with one component (and must not be with both).  The B forms are made on the
 * device and every slot is transformed as gsdr_acq_set_local_codes transforms its rows.  The handle
 * holds IQ-CAF codes -- plain runs are GSDR_E_STATE -- until another code setter is called.
 * GSDR_E_STATE before gsdr_acq_set_iq_caf; nsat = 0 or slots x nsat > max_prns is GSDR_E_ARG. */
int gsdr_acq_set_iq_codes(gsdr_acq* acq, const float* code_i, const float* code_q, const uint32_t* prn, uint32_t nsat);
/* nitems host items of fft_size samples of the handle's item type, fft_size apart; out
 * [nitems][nsat] records, fetched in one read-back.  Synchronous.  GSDR_E_STATE before both set
 * calls; nitems outside [1, max_blocks] is GSDR_E_ARG.  With gsdr_acq_set_profiling enabled the
 * forward pass is recorded in stage [0], the grid kernel in [1] and the input powers and the
 * finish kernel in [2]. */
int gsdr_acq_run_iq_caf(gsdr_acq* acq, const void* iq_host, uint32_t nitems, uint64_t stamp0,
    gsdr_acq_iq_caf_result* out);
/* The same on the ring's samples from first_sample, read in place. */
int gsdr_acq_run_iq_caf_stream(gsdr_acq* acq, gsdr_stream* stream, uint64_t first_sample, uint32_t nitems,
    uint64_t stamp0, gsdr_acq_iq_caf_result* out_host);
/* Debug/verification: the row records of one item, out [nsat][num_doppler_bins]. */
int gsdr_acq_dump_iq_caf_rows(gsdr_acq* acq, const void* iq_host, gsdr_acq_iq_caf_row* out);

/* ======================================================================== */
/* Tracking multicorrelator (Cpu_Multicorrelator_Real_Codes / Cpu_Multicorrelator) */
/* ======================================================================== */

typedef struct gsdr_corr gsdr_corr;

/* One correlation request: the 6 NCO parameters of
 * Carrier_wipeoff_multicorrelator_resampler (cpu_multicorrelator_real_codes.cc:103-126),
 * in the units dll_pll_veml_tracking passes them (do_correlation_step,
 * dll_pll_veml_tracking.cc:1064-1089): code terms already multiplied by samples/chip. */
typedef struct gsdr_corr_job
{
    int32_t channel;              /* correlator slot holding code + taps */
    int32_t n_samples;            /* signal_length_samples */
    int64_t sample_offset;        /* first input item of this job within the IQ buffer */
    float rem_carr_phase_rad;
    float carr_phase_step_rad;
    float carr_phase_rate_step_rad;
    float rem_code_phase_chips;
    float code_phase_step_chips;
    float code_phase_rate_step_chips;
} gsdr_corr_job;

/* init(max_signal_length_samples, n_correlators) for max_channels slots. */
int gsdr_corr_create(int device, int max_channels, int max_len, int max_taps, gsdr_corr** out);
void gsdr_corr_destroy(gsdr_corr* corr);

/* set_local_code_and_taps (cpu_multicorrelator_real_codes.cc:53-63); unlike the
 * reference (which keeps the caller's pointers) the code and shifts are copied
 * to the device, so the caller's arrays need not outlive the call. */
int gsdr_corr_set_local_code_and_taps(gsdr_corr* corr, int channel, int code_length_chips, const float* code,
    const float* shifts_chips, int n_taps);
/* Cpu_Multicorrelator::set_local_code_and_taps (complex replicas, cpu_multicorrelator.cc:54-62). */
int gsdr_corr_set_local_code_and_taps_complex(gsdr_corr* corr, int channel, int code_length_chips,
    const float* code_cf32, const float* shifts_chips, int n_taps);
/* set_high_dynamics_resampler (cpu_multicorrelator_real_codes.cc:161-165). */
int gsdr_corr_set_high_dynamics_resampler(gsdr_corr* corr, int channel, int enable);
/* Float association of the code-phase index (GSDR_ASSOC_*), default GSDR_ASSOC_AVX. */
int gsdr_corr_set_resampler_assoc(gsdr_corr* corr, int assoc);

/* Synchronous drop-in for one channel: Carrier_wipeoff_multicorrelator_resampler
 * (7-argument form) on host samples; writes n_taps complex<float> to corr_out_host.
 * item_type selects gr_complex, cshort or ibyte input (GSDR_ITEM_*). */
int gsdr_corr_run(gsdr_corr* corr, int channel, const void* sig_in_host, int item_type, float rem_carr_phase_rad,
    float carr_phase_step_rad, float carr_phase_rate_step_rad, float rem_code_phase_chips,
    float code_phase_step_chips, float code_phase_rate_step_chips, int signal_length_samples, float* corr_out_host);

/* Batched form: njobs jobs over one device IQ buffer (iq_dev, iq_items items of
 * item_type).  Writes, for job j, n_taps(channel) complex<float> at
 * out_dev + 2*j*max_taps.  jobs_host is copied; asynchronous on stream. */
int gsdr_corr_run_batch(gsdr_corr* corr, const gsdr_corr_job* jobs_host, int njobs, const void* iq_dev,
    int item_type, int64_t iq_items, float* out_dev, void* stream);

/* Same, with the job table already in device memory (graph-capturable). */
int gsdr_corr_run_batch_device(gsdr_corr* corr, const gsdr_corr_job* jobs_dev, int njobs, const void* iq_dev,
    int item_type, int64_t iq_items, float* out_dev, void* stream);

/* Multi-epoch schedule: n_epochs consecutive batches of jobs_per_epoch jobs
 * (jobs_dev holds n_epochs*jobs_per_epoch jobs, epoch-major).  Epoch e is one
 * launch queued behind epoch e-1 on the stream — the launch order a tracking
 * loop imposes — issued from native code.  Output of job j of epoch e at
 * out_dev + 2*(e*jobs_per_epoch + j)*max_taps. */
int gsdr_corr_run_epochs(gsdr_corr* corr, const gsdr_corr_job* jobs_dev, int jobs_per_epoch, int n_epochs,
    const void* iq_dev, int item_type, int64_t iq_items, float* out_dev, void* stream);

/* Kernel-time profiling with HIP events (see gsdr_acq_set_profiling). */
int gsdr_corr_set_profiling(gsdr_corr* corr, int enable);
int gsdr_corr_read_profile(gsdr_corr* corr, double* kernel_ms, uint32_t* launches);

/* Debug/verification: the resampled code indices of one channel, as the
 * kernel computes them (n_taps rows x n samples int32, host). */
int gsdr_corr_dump_indices(gsdr_corr* corr, int channel, float rem_code_phase_chips, float code_phase_step_chips,
    int n, int32_t* idx_host);

/* ======================================================================== */
/* Tracking — device-resident DLL/PLL loop (dll_pll_veml_tracking)           */
/* ======================================================================== */
/*
 * Replaces the per-epoch work of dll_pll_veml_tracking::general_work
 * (src/algorithms/tracking/gnuradio_blocks/dll_pll_veml_tracking.cc:1784-2152):
 * do_correlation_step (:1064-1089), run_dll_pll (:1092-1179),
 * update_tracking_vars (:1216-1287), cn0_and_tracking_lock_status (:970-1056),
 * the bit-synchronisation preamble search (acquire_secondary, :923-967) and the
 * state machine (states 2 and 4).  One handle owns a pool of channels; a launch
 * advances every active channel by up to max_epochs general_work calls over a
 * device-resident IQ buffer without returning to the host (one workgroup per
 * channel loops over its epochs: the tracking loop is sequential in time per
 * channel, parallel across channels).
 */
typedef struct gsdr_trk gsdr_trk;

#define GSDR_SIGNAL_GPS_1C 0 /* GPS L1 C/A (dll_pll_veml_tracking.cc:170-191) */
#define GSDR_SIGNAL_GAL_1B 1 /* Galileo E1 OS, VEML 5 taps, pilot (E1C) or data (E1B) tracking (:258-290) */
#define GSDR_SIGNAL_BDS_B1 2 /* BeiDou B1I D1 (NH secondary code) / D2 GEO (preamble) (:391-411, :762-795) */
#define GSDR_SIGNAL_GAL_5X 3 /* Galileo E5a, E/P/L, pilot (E5a-Q, per-PRN 100-chip secondary code) or data
                                (E5a-I, 20-chip secondary code) tracking (:289-319, :696-719) */
#define GSDR_SIGNAL_GPS_L5 4 /* GPS L5, E/P/L, pilot (L5-Q, 20-chip NH code) or data (L5-I, 10-chip NH code)
                                tracking (:210-244, :667-680) */

/* Mirrors Dll_Pll_Conf (src/algorithms/tracking/libs/dll_pll_conf.h:30-84);
 * gsdr_trk_conf_default() fills the reference defaults (incl. the gflags
 * defaults gnss_sdr_flags.cc:45-54 for cn0_samples, cn0_min, max_lock_fail,
 * max_carrier_lock_fail and carrier_lock_th). */
typedef struct gsdr_trk_conf
{
    double fs_in;
    double carrier_lock_th;
    uint32_t vector_length; /* correlation length; 0 -> round(fs_in / 1000) (gps_l1_ca_dll_pll_tracking.cc:42) */
    int32_t signal;         /* GSDR_SIGNAL_* */
    int32_t item_type;      /* GSDR_ITEM_* */
    uint32_t max_channels;
    float fll_bw_hz;
    float pll_bw_hz;
    float dll_bw_hz;
    float pll_bw_narrow_hz;
    float dll_bw_narrow_hz;
    float early_late_space_chips;
    float very_early_late_space_chips;
    float early_late_space_narrow_chips;
    float very_early_late_space_narrow_chips;
    float cn0_smoother_alpha;
    float carrier_lock_test_smoother_alpha;
    uint32_t pull_in_time_s;
    uint32_t bit_synchronization_time_limit_s;
    int32_t pll_filter_order;
    int32_t dll_filter_order;
    int32_t extend_correlation_symbols; /* coherent symbols per correlation after bit sync (state 3, :1989-2026) */
    int32_t cn0_samples;
    int32_t cn0_smoother_samples;
    int32_t carrier_lock_test_smoother_samples;
    int32_t cn0_min;
    int32_t max_code_lock_fail;
    int32_t max_carrier_lock_fail;
    int32_t enable_fll_pull_in;
    int32_t enable_fll_steady_state;
    int32_t carrier_aiding;
    int32_t high_dyn;    /* Dll_Pll_Conf::high_dyn: high-dynamics resampler/rotator + carrier/code rate
                            estimates from the step histories (dll_pll_veml_tracking.cc:1232-1284) */
    int32_t track_pilot; /* Dll_Pll_Conf::track_pilot (default 1); forced 0 for GPS L1 C/A and BeiDou B1I */
                         /* (:183, :402); Galileo E1, Galileo E5a and GPS L5 honour it */
    uint32_t smoother_length; /* Dll_Pll_Conf::smoother_length (default 10, at most 32): histories of 2x that */
} gsdr_trk_conf;

/* One general_work call of one channel (written for every call that ran a
 * correlation or changed state).  Gnss_Synchro fields as general_work fills them
 * (:2000-2017, :2121-2127) plus the loop state after the call. */
typedef struct gsdr_trk_epoch
{
    uint64_t sample_counter;       /* nitems_read(0) at the start of the call */
    int32_t state;                 /* d_state at the start of the call */
    int32_t consumed;              /* consume_each() count */
    float taps[10];                /* correlator outputs of the call: E,P,L (3 taps) or VE,E,P,L,VL */
    float rem_carr_phase_rad;      /* after the call */
    int32_t flags;                 /* GSDR_TRK_F_* */
    double carrier_doppler_hz;     /* Carrier_Doppler_hz */
    double code_freq_chips;
    double rem_code_phase_samples; /* Code_phase_samples */
    double acc_carrier_phase_rad;  /* Carrier_phase_rads */
    double cn0_db_hz;              /* CN0_dB_hz */
    double carrier_lock_test;
    double prompt_i;               /* Prompt_I (valid output only); with d_interchange_iq (E5a pilot, L5 data: */
    double prompt_q;               /* Prompt_Q  :242, :310) imag / real of d_P_data_accu (:2001-2010, :2054-2063) */
    double evm;                    /* EVM (fork indicator, :1027-1053) */
    float data_prompt[2];          /* pilot tracking: the data-component prompt of the call (d_Prompt_Data[0]) */
    float carrier_rate;            /* high_dyn: (float)d_carrier_phase_rate_step_rad after the call [rad/sample^2] */
    float code_rate;               /* high_dyn: (float)d_code_phase_rate_step_chips after the call [chips/sample^2] */
    /* log_data (dll_pll_veml_tracking.cc:1403-1500), valid when flags has GSDR_TRK_F_LOGGED: the
     * accumulator magnitudes |VE|, |E|, |P|, |L|, |VL| (VE/VL 0 without VEML) and the loop
     * errors as the dump writes them (static_cast<float> of the double members) */
    float log_accu[5];
    float carr_phase_error_hz, carr_error_filt_hz, code_error_chips, code_error_filt_chips;
    int32_t reserved;              /* 0 (keeps the record free of padding bytes) */
} gsdr_trk_epoch;

#define GSDR_TRK_F_VALID_OUTPUT 1 /* Flag_valid_symbol_output: a Gnss_Synchro was emitted */
#define GSDR_TRK_F_LOSS_OF_LOCK 2 /* event 3 (loss of lock), channel back to state 0 */
#define GSDR_TRK_F_PLL_180 4      /* Flag_PLL_180_deg_phase_locked */
#define GSDR_TRK_F_BIT_SYNC 8     /* preamble / bit synchronisation locked in this call (2 -> 4) */
#define GSDR_TRK_F_OVERRUN 16     /* with LOSS_OF_LOCK: the channel's next call starts before the oldest
                                     input item given (the ring moved past a stalled channel); the
                                     record carries the channel's position, the channel is in state 0 */
#define GSDR_TRK_F_LOGGED 32      /* the reference calls log_data() for this call (state 2 locked; states
                                     3/4 with a completed data symbol): the record's log_* fields are set */

void gsdr_trk_conf_default(gsdr_trk_conf* conf);
int gsdr_trk_create(int device, const gsdr_trk_conf* conf, gsdr_trk** out);
void gsdr_trk_destroy(gsdr_trk* trk);

/* start_tracking (:640-882) for channel ch with the acquisition results of
 * Gnss_Synchro (Acq_delay_samples, Acq_doppler_hz, Acq_samplestamp_samples) and
 * the PRN's tracking code replica (code_samples = samples_per_chip * code length
 * floats, e.g. gps_l1_ca_code_gen_float), followed by the state-1 pull-in call
 * (:1813-1844) executed at input position nitems_read.  *first_sample receives
 * the absolute input index of the first correlation (nitems_read + offset). */
int gsdr_trk_start(gsdr_trk* trk, int ch, uint32_t prn, const float* code, int code_samples,
    double acq_delay_samples, double acq_doppler_hz, uint64_t acq_samplestamp, uint64_t nitems_read,
    uint64_t* first_sample);
/* Pilot tracking (track_pilot, Galileo E1): the data component's replica for the
 * extra prompt correlator (d_correlator_data_cpu.set_local_code_and_taps,
 * dll_pll_veml_tracking.cc:681-689, e.g. galileo_e1_code_gen_sinboc11_float of
 * E1B), code_samples floats.  Call before gsdr_trk_start for that channel. */
int gsdr_trk_set_data_code(gsdr_trk* trk, int ch, const float* data_code, int code_samples);
/* Galileo E5a pilot tracking: the PRN's E5a-Q secondary code for channel ch
 * (d_secondary_code_string = GALILEO_E5A_Q_SECONDARY_CODE[PRN - 1],
 * dll_pll_veml_tracking.cc:703), len characters '0' / '1', 1 <= len <= 160.  Required
 * before gsdr_trk_start on such a handle (GSDR_E_STATE otherwise); handles of every
 * other signal and mode refuse it with GSDR_E_STATE.  The library ships no E5a table. */
int gsdr_trk_set_secondary_code(gsdr_trk* trk, int ch, const char* bits, int len);
/* stop_tracking: channel to state 0 (standby). */
int gsdr_trk_stop(gsdr_trk* trk, int ch);
/* msg_handler_telemetry_to_trk with tlm_event 1 (dll_pll_veml_tracking.cc:614-637,
 * port registered :142-147): a telemetry fault forces d_carrier_lock_fail_counter to
 * 200000, so the channel's next lock check past the CN0 fill (states 2 / 4) reports
 * the loss of lock (GSDR_TRK_F_LOSS_OF_LOCK).  Takes effect at the channel's next
 * call on the device (synchronous; ordered after the handle's last launch). */
int gsdr_trk_force_loss_of_lock(gsdr_trk* trk, int ch);

/* Advance every channel in states 2..4 by up to max_epochs general_work calls
 * over iq_dev, which holds iq_items items whose first item is absolute input
 * sample iq_first_sample.  A channel stops early when its next call would read
 * past the buffer.  out_dev: max_channels * max_epochs records, channel-major
 * (record e of channel c at c*max_epochs + e); n_out_dev: per-channel record
 * count (device).  Asynchronous on stream (NULL = the handle's own stream). */
int gsdr_trk_run_device(gsdr_trk* trk, const void* iq_dev, uint64_t iq_first_sample, uint64_t iq_items,
    uint32_t max_epochs, gsdr_trk_epoch* out_dev, uint32_t* n_out_dev, void* stream);

/* Ring form: every active channel advances by up to max_epochs calls over the
 * ring's newest contiguous window (gsdr_stream_span); a channel whose next call
 * needs items not pushed yet stops and continues on a later call, so pushing the
 * stream in any chunking gives the records of one contiguous run.  Asynchronous on
 * stream (NULL = the handle's own), ordered after the ring's pushes and before the
 * pushes that would overwrite the window. */
int gsdr_trk_run_stream(gsdr_trk* trk, gsdr_stream* ring, uint32_t max_epochs, gsdr_trk_epoch* out_dev,
    uint32_t* n_out_dev, void* stream);

/* Ring form with the records copied back to the host (synchronous; the
 * handle's own stream and record buffers): the tracking pool service's call. */
int gsdr_trk_run_stream_host(gsdr_trk* trk, gsdr_stream* ring, uint32_t max_epochs, gsdr_trk_epoch* out_host,
    uint32_t* n_out_host);

/* Asynchronous ring form for a host consumer (the pooled tracking blocks of
 * dll_pll_veml_tracking_pool_mi355x, which replace the per-channel general_work
 * round trips of dll_pll_veml_tracking.cc:1784-2152): gsdr_trk_run_stream on the
 * handle's stream into the handle's own submission buffers, the records and counts
 * copied into pinned host memory behind it; returns without waiting.  Up to two
 * submissions in flight (the second runs behind the first on the handle's stream, so
 * the GPU does not idle while the host collects); gsdr_trk_collect copies out the
 * oldest: out_host holds max_channels *
 * max_epochs records (channel-major; only the first n_out_host[c] of channel c are
 * written), n_out_host max_channels counts, *max_epochs
 * (may be NULL) the submission's max_epochs; wait != 0 waits for the copy, wait == 0
 * returns 1 without copying while it is in flight.  Submits on one handle are
 * serialised (each keeps its slot while it launches); a collect may run beside a
 * submit and sees only submissions that returned GSDR_OK. */
int gsdr_trk_submit_stream(gsdr_trk* trk, gsdr_stream* ring, uint32_t max_epochs);
int gsdr_trk_collect(gsdr_trk* trk, int wait, gsdr_trk_epoch* out_host, uint32_t* n_out_host, uint32_t* max_epochs);

/* Host form of the same call (synchronous): copies the records back. */
int gsdr_trk_run(gsdr_trk* trk, const void* iq_host, uint64_t iq_first_sample, uint64_t iq_items,
    uint32_t max_epochs, gsdr_trk_epoch* out_host, uint32_t* n_out_host);

/* Channel snapshot: current state, next input index, Doppler and CN0. */
int gsdr_trk_get_channel(gsdr_trk* trk, int ch, int32_t* state, uint64_t* next_sample, double* carrier_doppler_hz,
    double* cn0_db_hz);

/* Device-side copy of every channel's loop state into / out of snapshot slot
 * `slot` (0 or 1); asynchronous on stream.  Lets a caller replay the same input
 * span from the same loop state (benchmarks, what-if re-tracking). */
int gsdr_trk_save_state(gsdr_trk* trk, int slot, void* stream);
int gsdr_trk_restore_state(gsdr_trk* trk, int slot, void* stream);

/* Kalman-filter tracking loop (kf_tracking.cc of the reference): the discriminator ->
 * loop filter -> NCO chain of a handle is replaced by a four-state Kalman filter
 * (code-phase error [chips], carrier phase [rad], Doppler [Hz], Doppler rate [Hz/s])
 * driven by both discriminators; state machine, correlators, lock detectors and bit
 * synchronisation stay as they are.  The fields are the Kalman fields of Kf_Conf
 * (standard deviations; the filter uses their squares). */
typedef struct gsdr_trk_kf_conf
{
    double code_disc_sd_chips;   /* measurement noise R (pull-in; narrow tracking re-derives R from C/N0) */
    double carrier_disc_sd_rads;
    double code_phase_sd_chips;  /* process noise Q */
    double carrier_phase_sd_rad;
    double carrier_freq_sd_hz;
    double carrier_freq_rate_sd_hz_s;
    double init_code_phase_sd_chips;  /* initial covariance P0 */
    double init_carrier_phase_sd_rad;
    double init_carrier_freq_sd_hz;
    double init_carrier_freq_rate_sd_hz_s;
} gsdr_trk_kf_conf;

/* The Kf_Conf constructor's values: 0.2, 0.3, 0.15, 0.25, 0.6, 0.01, 0.5, 0.7, 5, 1. */
void gsdr_trk_kf_conf_default(gsdr_trk_kf_conf* conf);

/* Switches the handle to the Kalman loop, for every channel and for good.  Only while
 * no channel has been started (GSDR_E_STATE otherwise); a negative or non-finite value
 * is GSDR_E_ARG; a handle created with high_dyn is GSDR_E_UNSUPPORTED (kf_tracking's
 * high-dynamics branch is not implemented).  A refused call leaves the handle as it
 * was.  In Kalman mode fll_bw_hz, pll_bw*, dll_bw*, the filter orders, enable_fll_* and
 * carrier_aiding are ignored: the code frequency is always chip_rate + doppler *
 * chip_rate / carrier.  The four log fields of gsdr_trk_epoch carry what
 * kf_tracking::log_data dumps in their place (carrier discriminator [Hz], (float)x(2),
 * code discriminator, (float) code error estimate); evm, carrier_rate and code_rate
 * are 0. */
int gsdr_trk_set_kf(gsdr_trk* trk, const gsdr_trk_kf_conf* conf);

/* The filter's state x (4) and covariance P (16, row-major) of channel ch; synchronous,
 * ordered after the handle's last launch like gsdr_trk_get_channel.  GSDR_E_STATE on a
 * handle that is not in Kalman mode. */
int gsdr_trk_get_kf_state(gsdr_trk* trk, int ch, double x[4], double P[16]);

/* Kernel-time profiling with HIP events (see gsdr_acq_set_profiling). */
int gsdr_trk_set_profiling(gsdr_trk* trk, int enable);

/* Compute-unit partitioning (MI355X: 256 CUs in 8 XCDs).  Recreates the handle's
 * own stream (the one used when a call passes stream = NULL) restricted to the CUs
 * whose bits are set in mask[0..n_words) -- bit i selects CU i/8 of XCD i%8
 * (hipExtStreamCreateWithCUMask numbering).  A latency-bound tracking pool can so
 * own a few CUs while the throughput-bound acquisition grid fills the rest.
 * n_words = 0 restores an unrestricted stream. */
int gsdr_acq_set_cu_mask(gsdr_acq* acq, const uint32_t* mask, int n_words);
int gsdr_trk_set_cu_mask(gsdr_trk* trk, const uint32_t* mask, int n_words);
int gsdr_trk_read_profile(gsdr_trk* trk, double* kernel_ms, uint32_t* launches);

#ifdef __cplusplus
}
#endif

#endif /* GSDR_H */
