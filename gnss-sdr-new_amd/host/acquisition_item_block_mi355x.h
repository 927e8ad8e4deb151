// What the item-wise acquisition blocks on the MI355X engine have in common: the blocks whose
// general_work takes whole items through the reference's states 0 (idle), 1 (search) and two
// terminal states (pcps_pair_, pcps_quicksync_, pcps_tong_acquisition_mi355x.h,
// galileo_e5a_noncoherent_iq_acquisition_caf_block_mi355x.h).  The reference repeats this text in
// every one of its blocks: the synchro clear and the Doppler-bin count of init(), the restart of
// set_state(1) and of state 0, the terminal states' event.  Here it stands once, beside what the
// MI355X side adds to each block alike: the engine handle, the device ring and the end-of-item
// stamp.  A block keeps its conf and constructor checks, its code upload, the mode calls of its
// init() and the state-1 body of its work().  A new item-wise mode starts as a class derived from
// this one.
#ifndef GSDR_HOST_ACQUISITION_ITEM_BLOCK_MI355X_H
#define GSDR_HOST_ACQUISITION_ITEM_BLOCK_MI355X_H

#include <cstdint>
#include <functional>
#include <string>

#include "gnss_synchro.h"
#include "gsdr.h"

// The rows of the grid as every init() and calculate_threshold() of the reference counts them:
// -doppler_max, -doppler_max + doppler_step, ... up to doppler_max.  The loop does not end with
// a zero step: the caller refuses that first.
uint32_t acquisition_doppler_bins(uint32_t doppler_max, uint32_t doppler_step);

class acquisition_item_block_mi355x
{
public:
    virtual ~acquisition_item_block_mi355x();
    acquisition_item_block_mi355x(const acquisition_item_block_mi355x&) = delete;
    acquisition_item_block_mi355x& operator=(const acquisition_item_block_mi355x&) = delete;

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    uint32_t mag() const { return static_cast<uint32_t>(d_mag); }
    // counts the Doppler bins and creates the grid: here, the engine handle
    virtual void init() = 0;
    void set_active(bool active) { d_active = active; }
    void set_state(int32_t state);
    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_threshold(float threshold);
    void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }
    void set_event_handler(std::function<void(int)> h) { d_events = std::move(h); }
    // Ring path: the items work() is given are also samples [origin + d_sample_counter, ...)
    // of the device ring, and state 1 reads its items there in place.
    void set_ring(gsdr_stream* ring, uint64_t origin);

    int state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    float threshold() const { return d_threshold; }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    float mag_value() const { return d_mag; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }

protected:
    // name: the prefix of the block's messages; item_samples: the samples of one item of work()
    acquisition_item_block_mi355x(const char* name, int device, int64_t fs_in, uint32_t doppler_max, uint32_t item_samples);

    [[noreturn]] void fail() const;  // throws the engine's last error under the block's name
    // init(): the synchro's acquisition fields, d_mag and d_input_power cleared
    void clear_synchro();
    // init(): a conf for a grid of fft_size points over d_num_doppler_bins rows (counted here),
    // one PRN slot, one block per call and 1 ms codes: max_prns, max_blocks, sampled_ms and
    // ms_per_code are the block's to change
    gsdr_acq_conf grid_conf(uint32_t fft_size, uint32_t samples_per_code);
    // init(): the engine of that conf in place of the one held, with the grid's carrier model
    void create_engine(const gsdr_acq_conf& conf, int wipeoff_mode);
    // set_state(1) and state 0 with d_active: the synchro fields and the statistics cleared, then
    // the block's own counters (restart_counters)
    void restart();
    virtual void restart_counters() = 0;
    // state 0 of work(): consumes the items, and starts a search if one was asked for
    int idle_step(int ninput_items);
    // the terminal states of work(): the event (1 positive, 2 negative), the synchro into
    // monitor_out for a positive acquisition where the block is given one, back to state 0
    int terminal_step(bool positive, int ninput_items, Gnss_Synchro* monitor_out = nullptr, int* noutput_items = nullptr);
    // state 1: a winning record into the synchro.  The engine stamps the item's first sample; the
    // reference advances its counter before the grid, so its stamp is the item's end
    void take_winner(double acq_delay_samples, int32_t doppler_hz, uint64_t item_first_sample);

    const std::string d_name;
    const int d_device;
    const int64_t d_fs_in;
    gsdr_acq* d_engine{nullptr};
    gsdr_stream* d_ring{nullptr};
    uint64_t d_ring_origin{0};
    Gnss_Synchro* d_gnss_synchro{nullptr};
    std::function<void(int)> d_events;
    uint64_t d_sample_counter{0};
    float d_threshold{0.0F};
    float d_mag{0.0F};
    float d_input_power{0.0F};
    float d_test_statistics{0.0F};
    int32_t d_state{0};
    uint32_t d_channel{0};
    uint32_t d_doppler_max;
    uint32_t d_doppler_step{0};
    uint32_t d_num_doppler_bins{0};
    const uint32_t d_item_samples;
    bool d_active{false};
    // pcps_quicksync_acquisition_cc.cc:199-221: its set_state(1) also sets d_active
    bool d_set_state_activates{false};
    // the Tong counter runs on the device: its threshold goes to the engine as well
    bool d_threshold_on_engine{false};
};

#endif
