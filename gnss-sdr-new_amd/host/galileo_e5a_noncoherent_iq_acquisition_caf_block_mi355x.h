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
#include <functional>
#include <vector>

#include "gnss_synchro.h"
#include "gsdr.h"

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

class galileo_e5a_noncoherentIQ_acquisition_caf_mi355x
{
public:
    explicit galileo_e5a_noncoherentIQ_acquisition_caf_mi355x(const E5a_Iq_Caf_Acq_Conf& conf, int device = 0);
    ~galileo_e5a_noncoherentIQ_acquisition_caf_mi355x();
    galileo_e5a_noncoherentIQ_acquisition_caf_mi355x(const galileo_e5a_noncoherentIQ_acquisition_caf_mi355x&) = delete;
    galileo_e5a_noncoherentIQ_acquisition_caf_mi355x& operator=(const galileo_e5a_noncoherentIQ_acquisition_caf_mi355x&) =
        delete;

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    uint32_t mag() const { return static_cast<uint32_t>(d_mag); }
    // counts the Doppler bins and creates the wipe-offs (:211-255): here, the engine handle
    void init();
    // :160-208: fft_size samples each; codeQ is read with both components only
    void set_local_code(std::complex<float>* codeI, std::complex<float>* codeQ);
    void set_active(bool active) { d_active = active; }
    void set_state(int32_t state);
    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_threshold(float threshold) { d_threshold = threshold; }
    void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }
    void set_event_handler(std::function<void(int)> h) { d_events = std::move(h); }
    // Ring path: the items work() is given are also samples [origin + d_sample_counter, ...)
    // of the device ring, and state 1 reads its items there in place.
    void set_ring(gsdr_stream* ring, uint64_t origin);

    // general_work: `in` holds ninput_items items of fft_size() samples; returns the items
    // consumed (consume_each).  monitor_out, when given, receives the Gnss_Synchro of a positive
    // acquisition if the monitor output is enabled, and *noutput_items how many (0 or 1).
    int work(const std::complex<float>* in, int ninput_items, Gnss_Synchro* monitor_out = nullptr,
        int* noutput_items = nullptr);

    int state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    float threshold() const { return d_threshold; }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    float mag_value() const { return d_mag; }
    uint32_t well_count() const { return d_well_count; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t coherent_ms() const { return d_sampled_ms; }
    uint32_t batch_items() const { return d_batch; }
    bool both_signal_components() const { return d_both_signal_components; }
    const gsdr_acq_iq_caf_result& last_record() const { return d_last; }

private:
    void upload_code();
    void restart();

    E5a_Iq_Caf_Acq_Conf d_conf;
    int d_device;
    gsdr_acq* d_engine{nullptr};
    gsdr_stream* d_ring{nullptr};
    uint64_t d_ring_origin{0};
    Gnss_Synchro* d_gnss_synchro{nullptr};
    std::function<void(int)> d_events;
    std::vector<std::complex<float>> d_code_i, d_code_q;
    std::vector<gsdr_acq_iq_caf_result> d_records;
    gsdr_acq_iq_caf_result d_last{};
    uint64_t d_sample_counter{0};
    float d_threshold{0.0F};
    float d_mag{0.0F};
    float d_input_power{0.0F};
    float d_test_statistics{0.0F};
    int32_t d_state{0};
    int32_t d_CAF_window_hz;
    uint32_t d_channel{0};
    uint32_t d_doppler_max;
    uint32_t d_doppler_step{250};  // :88
    uint32_t d_samples_per_code;
    uint32_t d_fft_size;
    uint32_t d_sampled_ms;  // 1 with Zero_padding (:104-111)
    uint32_t d_max_dwells;
    uint32_t d_well_count{0};
    uint32_t d_batch;  // items per engine call: no attempt takes more than max_dwells
    uint32_t d_num_doppler_bins{0};
    bool d_bit_transition_flag;
    bool d_both_signal_components;
    bool d_active{false};
    bool d_enable_monitor_output;
};

#endif
