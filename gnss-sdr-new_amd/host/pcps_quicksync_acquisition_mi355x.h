// pcps_quicksync_acquisition_cc on the MI355X engine
// (src/algorithms/acquisition/gnuradio_blocks/pcps_quicksync_acquisition_cc.cc).  With folding
// factor p an item is sampled_ms * samples_per_ms = p samples_per_code samples; the grid runs
// on samples_per_code / p points and the p delays its winner stands for are told apart by p
// correlations in time (include/gsdr.h, "QuickSync acquisition").
// The GNU Radio plumbing is replaced by work() over items and an event callback (the "events"
// message port: 1 positive, 2 negative).  One gsdr_acq_run_quicksync (or
// gsdr_acq_run_quicksync_stream on the device ring, set_ring) per state-1 call.  Kept as the
// reference has them: d_mag, d_input_power and d_test_statistics are zeroed in every state-1
// call (:288-291), so every dwell is a grid of its own and, with bit_transition_flag, the
// decision after max_dwells is taken on the last dwell's statistic alone; a doppler_step of 0
// becomes 250 in init() (:173-176); Acq_samplestamp_samples is the end of the item (:293, :417).
// Refused with a message where the reference reads or writes out of bounds or drops samples:
// a folding factor outside [2, 16], samples_per_code no multiple of it, an item that is not
// p samples_per_code samples.  Not mirrored: d_dump (:426-440).
#ifndef GSDR_HOST_PCPS_QUICKSYNC_ACQUISITION_MI355X_H
#define GSDR_HOST_PCPS_QUICKSYNC_ACQUISITION_MI355X_H

#include <complex>
#include <cstdint>
#include <vector>

#include "acquisition_item_block_mi355x.h"

// the arguments of pcps_quicksync_make_acquisition_cc
struct QuickSync_Acq_Conf
{
    uint32_t folding_factor{4};
    uint32_t sampled_ms{4};
    uint32_t max_dwells{1};
    uint32_t doppler_max{5000};
    int64_t fs_in{4000000};
    int32_t samples_per_ms{4000};
    int32_t samples_per_code{4000};
    bool bit_transition_flag{false};
};

class pcps_quicksync_acquisition_mi355x : public acquisition_item_block_mi355x
{
public:
    explicit pcps_quicksync_acquisition_mi355x(const QuickSync_Acq_Conf& conf, int device = 0);

    // counts the Doppler bins and creates the grid (:160-196): here, the engine handle
    void init() override;
    // :135-157: samples_per_code samples, unfolded
    void set_local_code(std::complex<float>* code);

    // general_work: `in` holds ninput_items items of item_samples() samples; returns the items
    // consumed (consume_each).
    int work(const std::complex<float>* in, int ninput_items);

    uint32_t fft_size() const { return d_fft_size; }
    uint32_t item_samples() const { return d_item_samples; }
    uint32_t folding_factor() const { return d_folding_factor; }
    const gsdr_acq_quicksync_result& last_record() const { return d_last; }

private:
    void upload_code();
    void restart_counters() override;

    std::vector<std::complex<float>> d_code;
    gsdr_acq_quicksync_result d_last{};
    uint32_t d_folding_factor;
    uint32_t d_max_dwells;
    uint32_t d_well_count{0};
    uint32_t d_samples_per_code;
    uint32_t d_fft_size;
    bool d_bit_transition_flag;
};

#endif
