// pcps_tong_acquisition_cc on the MI355X engine
// (src/algorithms/acquisition/gnuradio_blocks/pcps_tong_acquisition_cc.cc): the variable-dwell
// detector.  An item is sampled_ms * samples_per_ms samples; the grid of a sequence of items is
// kept on the device and the Tong counter runs there too (include/gsdr.h, "Tong acquisition").
// The GNU Radio plumbing is replaced by work() over items, an event callback (the "events"
// message port: 1 positive, 2 negative) and an optional Gnss_Synchro output item (the monitor
// output of state 2).
// Where the reference handles one item per state-1 call, this block hands every whole item it
// is offered (up to what the sequence can still take) to one gsdr_acq_run_tong (or
// gsdr_acq_run_tong_stream on the device ring, set_ring) and consumes up to and including the
// first item that ends the sequence: the state, counters, sample counter and synchro fields
// after the call are those the reference has after as many calls of one item.  Offered one item
// per call it is the reference call for call.
// Kept as the reference has them: the stamp is the end of the item (:272, :330); the
// tong_max_dwells rule comes after the counter and overrides a positive of the same dwell
// (:369-372).  Refused with a message where the reference's unsigned counter would wrap or never
// meet its '==': tong_init_val 0 or >= tong_max_val, and tong_max_dwells 0.  A doppler_step of 0,
// with which the reference's init() never returns (:168-173), is refused too.  Not mirrored:
// d_dump (:335-346).
#ifndef GSDR_HOST_PCPS_TONG_ACQUISITION_MI355X_H
#define GSDR_HOST_PCPS_TONG_ACQUISITION_MI355X_H

#include <complex>
#include <cstdint>
#include <vector>

#include "acquisition_item_block_mi355x.h"

// the arguments of pcps_tong_make_acquisition_cc
struct Tong_Acq_Conf
{
    uint32_t sampled_ms{1};
    uint32_t doppler_max{5000};
    int64_t fs_in{4000000};
    int32_t samples_per_ms{4000};
    int32_t samples_per_code{4000};
    uint32_t tong_init_val{1};
    uint32_t tong_max_val{2};
    uint32_t tong_max_dwells{3};
    bool enable_monitor_output{false};
};

class pcps_tong_acquisition_mi355x : public acquisition_item_block_mi355x
{
public:
    explicit pcps_tong_acquisition_mi355x(const Tong_Acq_Conf& conf, int device = 0);

    // counts the Doppler bins and creates the grid (:153-185): here, the engine handle
    void init() override;
    // :142-150: fft_size samples
    void set_local_code(std::complex<float>* code);

    // general_work: `in` holds ninput_items items of fft_size() samples; returns the items
    // consumed (consume_each).  monitor_out, when given, receives the Gnss_Synchro of a positive
    // acquisition if the monitor output is enabled, and *noutput_items how many (0 or 1).
    int work(const std::complex<float>* in, int ninput_items, Gnss_Synchro* monitor_out = nullptr,
        int* noutput_items = nullptr);

    uint32_t dwell_count() const { return d_dwell_count; }
    uint32_t tong_count() const { return d_tong_count; }
    uint32_t fft_size() const { return d_item_samples; }
    uint32_t batch_items() const { return d_batch; }
    const gsdr_acq_tong_result& last_record() const { return d_last; }

private:
    void upload_code();
    void restart_counters() override;

    std::vector<std::complex<float>> d_code;
    std::vector<gsdr_acq_tong_result> d_records;
    gsdr_acq_tong_result d_last{};
    uint32_t d_samples_per_code;
    uint32_t d_dwell_count{0};
    uint32_t d_tong_init_val;
    uint32_t d_tong_max_val;
    uint32_t d_tong_max_dwells;
    uint32_t d_tong_count;
    uint32_t d_batch;  // items per engine call: no sequence takes more than tong_max_dwells
    bool d_enable_monitor_output;
};

#endif
