// pcps_acquisition_fine_doppler_cc on the MI355X engine: the block's state machine as
// the reference runs it (general_work,
// src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition_fine_doppler_cc.cc:456-607),
// with the GNU Radio plumbing replaced by work() and an event callback (the "events"
// message port: 1 positive, 2 negative).
//   coarse stage  compute_and_accumulate_grid (:297-343) + compute_CAF (:213-282): a
//                 handle with num_doppler_bins = floor(2 doppler_max / doppler_step) (:134),
//                 pfa = 0 (first / second peak) and the block's max_dwells, one
//                 gsdr_acq_run_dwell per state-1 call; the block decides once, on the grid
//                 accumulated over all max_dwells blocks (:497-515)
//   fine stage    estimate_Doppler (:346-419): gsdr_acq_fine_doppler on the 10 ms buffer,
//                 or gsdr_acq_fine_doppler_stream on the device ring's window (set_ring)
#ifndef GSDR_HOST_PCPS_ACQUISITION_FINE_DOPPLER_MI355X_H
#define GSDR_HOST_PCPS_ACQUISITION_FINE_DOPPLER_MI355X_H

#include <complex>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "acq_conf.h"
#include "gnss_synchro.h"
#include "gsdr.h"

class pcps_acquisition_fine_doppler_mi355x
{
public:
    explicit pcps_acquisition_fine_doppler_mi355x(const Acq_Conf& conf, int device = 0);
    ~pcps_acquisition_fine_doppler_mi355x();
    pcps_acquisition_fine_doppler_mi355x(const pcps_acquisition_fine_doppler_mi355x&) = delete;
    pcps_acquisition_fine_doppler_mi355x& operator=(const pcps_acquisition_fine_doppler_mi355x&) = delete;

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    uint32_t mag() const { return static_cast<uint32_t>(d_test_statistics); }
    void init();
    void set_local_code(std::complex<float>* code);
    void set_active(bool active) { d_active = active; }
    void set_state(int state);
    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_threshold(float threshold) { d_threshold = threshold; }
    void set_doppler_max(uint32_t doppler_max) { d_config_doppler_max = static_cast<int32_t>(doppler_max); }
    // creates the search grid (:129-144): here, the engine handle of the coarse stage
    void set_doppler_step(uint32_t doppler_step);
    void set_event_handler(std::function<void(int)> h) { d_events = std::move(h); }
    bool start();
    // Ring path: the items work() is given are also items [origin + d_sample_counter, ...)
    // of the device ring, so the fine stage reads its 10 ms window there in place
    // instead of copying it (the state-3 copies of :518-538 are not made).
    void set_ring(gsdr_stream* ring, uint64_t origin);

    // general_work: `in` holds noutput_items items (at least one block of d_fft_size);
    // returns the number consumed (consume_each).
    int work(const std::complex<float>* in, int noutput_items);

    int state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    float threshold() const { return d_threshold; }
    float test_statistics() const { return d_test_statistics; }
    int num_doppler_points() const { return d_num_doppler_points; }
    int fft_size() const { return d_fft_size; }
    int64_t dump_number() const { return d_dump_number; }
    const std::string& last_dump_path() const { return d_last_dump; }
    const gsdr_acq_fine_result& last_fine_result() const { return d_fine; }

private:
    void reset_grid();
    float compute_CAF();
    int estimate_Doppler();
    void dump_results(int effective_fft_size);

    Acq_Conf acq_parameters;
    int d_device;
    gsdr_acq* d_engine{nullptr};
    gsdr_stream* d_ring{nullptr};
    uint64_t d_ring_origin{0};
    uint64_t d_window_first{0};  // d_sample_counter at the first dwell of the attempt
    Gnss_Synchro* d_gnss_synchro{nullptr};
    std::function<void(int)> d_events;
    std::vector<std::complex<float>> d_code;
    std::vector<std::complex<float>> d_10_ms_buffer;
    std::vector<float> d_grid, d_grid_tmp;  // dump: fft_size x num_doppler_points, column-major (grid_)
    gsdr_acq_result d_coarse{};
    gsdr_acq_fine_result d_fine{};
    std::string d_dump_filename;
    std::string d_last_dump;
    int64_t d_fs_in;
    int64_t d_dump_number{0};
    uint64_t d_sample_counter{0};
    float d_threshold{0.0F};
    float d_test_statistics{0.0F};
    int d_positive_acq{0};
    int d_state{0};
    int d_samples_per_ms;
    int d_max_dwells;
    int d_config_doppler_max;
    int d_num_doppler_points{0};
    int d_well_count{0};
    int d_n_samples_in_buffer{0};
    int d_fft_size;
    unsigned int d_doppler_step{0};
    unsigned int d_channel{0};
    unsigned int d_dump_channel{0};
    bool d_active{false};
    bool d_dump;
};

#endif
