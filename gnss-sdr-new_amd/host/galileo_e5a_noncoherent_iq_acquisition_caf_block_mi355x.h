// galileo_e5a_noncoherentIQ_acquisition_caf_cc on the MI355X engine
// (src/algorithms/acquisition/gnuradio_blocks/galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc):
// the E5a search over the data and pilot replicas, their first-period-inverted forms with 2 or 3 ms
// of coherent integration, the non-coherent sum of the two chosen rows and the optional CAF filter
// over the Doppler rows.  The grid, the selection, the sum and the filter run on the device
// (include/gsdr.h, "E5a non-coherent IQ acquisition with CAF filter"); the dwell rule is here.
// The GNU Radio plumbing is replaced by work() over items of fft_size samples, an event callback
// (the "events" message port: 1 positive, 2 negative) and an optional Gnss_Synchro output item
// (the monitor output of state 3).
// The reference spends three calls on a dwell: state 1 fills its buffer with fft_size samples,
// a second state-1 call finds it full, state 2 runs the grid (:328-359, :702).  Between them they
// consume exactly fft_size samples.  This block takes whole items: a state-1 call hands every item
// it is offered, up to what the attempt can still take, to one gsdr_acq_run_iq_caf (or
// gsdr_acq_run_iq_caf_stream on the device ring, set_ring) and folds the records dwell by dwell:
// the state, counters, sample counter and synchro fields after the call are those the reference
// has after as many dwells.  State 2 is therefore never seen from outside; states 0, 1, 3 and 4
// are the reference's.
// Kept as the reference has them: the stamp is the end of the item (:359, :563);
// d_test_statistics survives from dwell to dwell of an attempt (:559); with the filter on, every
// dwell's CAF Doppler overwrites Acq_doppler_hz whether or not its winner took over (:672).
// Refused with a message where the reference would divide by zero or index outside its vectors:
// a CAF window below 2 doppler_step or wider than the grid; and max_dwells 0, with which it never
// decides.  Not mirrored: d_dump.
#ifndef GSDR_HOST_GALILEO_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_BLOCK_MI355X_H
#define GSDR_HOST_GALILEO_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_BLOCK_MI355X_H

#include <complex>
#include <cstdint>
#include <vector>

#include "acquisition_item_block_mi355x.h"

// the arguments of galileo_e5a_noncoherentIQ_make_acquisition_caf_cc
struct E5a_Iq_Caf_Acq_Conf
{
    uint32_t sampled_ms{1};
    uint32_t max_dwells{1};
    uint32_t doppler_max{5000};
    int64_t fs_in{32000000};
    int32_t samples_per_ms{32000};
    int32_t samples_per_code{32000};
    bool bit_transition_flag{false};
    bool both_signal_components{false};
    int32_t CAF_window_hz{0};
    int32_t Zero_padding{0};
    bool enable_monitor_output{false};
};

class galileo_e5a_noncoherentIQ_acquisition_caf_mi355x : public acquisition_item_block_mi355x
{
public:
    explicit galileo_e5a_noncoherentIQ_acquisition_caf_mi355x(const E5a_Iq_Caf_Acq_Conf& conf, int device = 0);

    // counts the Doppler bins and creates the wipe-offs (:211-255): here, the engine handle
    void init() override;
    // :160-208: fft_size samples each; codeQ is read with both components only
    void set_local_code(std::complex<float>* codeI, std::complex<float>* codeQ);

    // general_work: `in` holds ninput_items items of fft_size() samples; returns the items
    // consumed (consume_each).  monitor_out, when given, receives the Gnss_Synchro of a positive
    // acquisition if the monitor output is enabled, and *noutput_items how many (0 or 1).
    int work(const std::complex<float>* in, int ninput_items, Gnss_Synchro* monitor_out = nullptr,
        int* noutput_items = nullptr);

    uint32_t well_count() const { return d_well_count; }
    uint32_t fft_size() const { return d_item_samples; }
    uint32_t coherent_ms() const { return d_sampled_ms; }
    uint32_t batch_items() const { return d_batch; }
    bool both_signal_components() const { return d_both_signal_components; }
    const gsdr_acq_iq_caf_result& last_record() const { return d_last; }

private:
    void upload_code();
    void restart_counters() override;

    std::vector<std::complex<float>> d_code_i, d_code_q;
    std::vector<gsdr_acq_iq_caf_result> d_records;
    gsdr_acq_iq_caf_result d_last{};
    int32_t d_CAF_window_hz;
    uint32_t d_samples_per_code;
    uint32_t d_sampled_ms;  // 1 with Zero_padding (:104-111)
    uint32_t d_max_dwells;
    uint32_t d_well_count{0};
    uint32_t d_batch;  // items per engine call: no attempt takes more than max_dwells
    bool d_bit_transition_flag;
    bool d_both_signal_components;
    bool d_enable_monitor_output;
};

#endif
