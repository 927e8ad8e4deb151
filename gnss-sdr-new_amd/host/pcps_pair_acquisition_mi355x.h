// pcps_cccwsr_acquisition_cc and galileo_pcps_8ms_acquisition_cc on the MI355X engine: one
// block for both, since their general_work is the same text
// (src/algorithms/acquisition/gnuradio_blocks/pcps_cccwsr_acquisition_cc.cc:205-436,
// galileo_pcps_8ms_acquisition_cc.cc:195-420) but for two things, which the policy names:
//   how the two replicas are made    CCCWSR: set_local_code(code_data, code_pilot), searched
//                                    as data - j pilot and data + j pilot (the reference's
//                                    d_correlation_plus / _minus); 8 ms: set_local_code(code),
//                                    code A as given and code B with samples
//                                    [samples_per_code, 2 samples_per_code) negated
//   whether d_mag survives a dwell   CCCWSR keeps d_mag and the synchro fields from dwell to
//                                    dwell (:157, :191, :334-341); the 8 ms block zeroes
//                                    d_mag in every state-1 call (:238-239)
// The GNU Radio plumbing is replaced by work() over items of fft_size samples and an event
// callback (the "events" message port: 1 positive, 2 negative).  One gsdr_acq_run_pairs
// (or gsdr_acq_run_pairs_stream on the device ring, set_ring) per state-1 call; the carry
// is done here, since one dwell arrives per call.  Not mirrored: d_dump, which writes one
// file per Doppler row of whatever the last inverse transform left (:344-355).
#ifndef GSDR_HOST_PCPS_PAIR_ACQUISITION_MI355X_H
#define GSDR_HOST_PCPS_PAIR_ACQUISITION_MI355X_H

#include <complex>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "gnss_synchro.h"
#include "gsdr.h"

// the arguments of pcps_cccwsr_make_acquisition_cc / galileo_pcps_8ms_make_acquisition_cc
struct Pair_Acq_Conf
{
    enum Policy
    {
        CCCWSR,   // two codes, d_mag carried
        PCPS_8MS  // one code as [c, c] and [c, -c], d_mag per dwell
    } policy{CCCWSR};
    uint32_t sampled_ms{4};
    uint32_t max_dwells{1};
    uint32_t doppler_max{5000};
    int64_t fs_in{4000000};
    int32_t samples_per_ms{4000};
    int32_t samples_per_code{16000};
    int wipeoff_mode{GSDR_WIPE_EXACT};  // MI355X extension: the carrier model of the grid
};

class pcps_pair_acquisition_mi355x
{
public:
    explicit pcps_pair_acquisition_mi355x(const Pair_Acq_Conf& conf, int device = 0);
    ~pcps_pair_acquisition_mi355x();
    pcps_pair_acquisition_mi355x(const pcps_pair_acquisition_mi355x&) = delete;
    pcps_pair_acquisition_mi355x& operator=(const pcps_pair_acquisition_mi355x&) = delete;

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    uint32_t mag() const { return static_cast<uint32_t>(d_mag); }
    // counts the Doppler bins and creates the grid (:147-177): here, the engine handle
    void init();
    // CCCWSR (:126-144): fft_size samples each
    void set_local_code(std::complex<float>* code_data, std::complex<float>* code_pilot);
    // 8 ms (galileo_pcps_8ms_acquisition_cc.cc:114-135): fft_size samples
    void set_local_code(std::complex<float>* code);
    void set_active(bool active) { d_active = active; }
    void set_state(int32_t state);
    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_threshold(float threshold) { d_threshold = threshold; }
    void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }
    void set_event_handler(std::function<void(int)> h) { d_events = std::move(h); }
    // Ring path: the items work() is given are also samples [origin + d_sample_counter, ...)
    // of the device ring, and state 1 reads its item there in place.
    void set_ring(gsdr_stream* ring, uint64_t origin);

    // general_work: `in` holds ninput_items items of fft_size samples; returns the items
    // consumed (consume_each).
    int work(const std::complex<float>* in, int ninput_items);

    int state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    float threshold() const { return d_threshold; }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    float mag_value() const { return d_mag; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t fft_size() const { return d_fft_size; }
    const gsdr_acq_pair_result& last_record() const { return d_last; }

private:
    void upload_codes();
    void restart();

    Pair_Acq_Conf d_conf;
    int d_device;
    gsdr_acq* d_engine{nullptr};
    gsdr_stream* d_ring{nullptr};
    uint64_t d_ring_origin{0};
    Gnss_Synchro* d_gnss_synchro{nullptr};
    std::function<void(int)> d_events;
    std::vector<std::complex<float>> d_first, d_second;
    gsdr_acq_pair_result d_last{};
    uint64_t d_sample_counter{0};
    float d_threshold{0.0F};
    float d_mag{0.0F};
    float d_input_power{0.0F};
    float d_test_statistics{0.0F};
    int32_t d_state{0};
    uint32_t d_channel{0};
    uint32_t d_doppler_max;
    uint32_t d_doppler_step{0};
    uint32_t d_max_dwells;
    uint32_t d_well_count{0};
    uint32_t d_fft_size;
    uint32_t d_samples_per_code;
    uint32_t d_num_doppler_bins{0};
    bool d_active{false};
};

#endif
