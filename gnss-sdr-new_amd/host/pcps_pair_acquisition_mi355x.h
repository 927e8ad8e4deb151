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
#include <vector>

#include "acquisition_item_block_mi355x.h"

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

class pcps_pair_acquisition_mi355x : public acquisition_item_block_mi355x
{
public:
    explicit pcps_pair_acquisition_mi355x(const Pair_Acq_Conf& conf, int device = 0);

    // counts the Doppler bins and creates the grid (:147-177): here, the engine handle
    void init() override;
    // CCCWSR (:126-144): fft_size samples each
    void set_local_code(std::complex<float>* code_data, std::complex<float>* code_pilot);
    // 8 ms (galileo_pcps_8ms_acquisition_cc.cc:114-135): fft_size samples
    void set_local_code(std::complex<float>* code);

    // general_work: `in` holds ninput_items items of fft_size samples; returns the items
    // consumed (consume_each).
    int work(const std::complex<float>* in, int ninput_items);

    uint32_t fft_size() const { return d_item_samples; }
    const gsdr_acq_pair_result& last_record() const { return d_last; }

private:
    void upload_codes();
    void restart_counters() override;

    Pair_Acq_Conf d_conf;
    std::vector<std::complex<float>> d_first, d_second;
    gsdr_acq_pair_result d_last{};
    uint32_t d_max_dwells;
    uint32_t d_well_count{0};
    uint32_t d_samples_per_code;
};

#endif
