#include "pcps_quicksync_acquisition_mi355x.h"

#include <stdexcept>
#include <string>

// pcps_quicksync_acquisition_cc.cc:54-112
pcps_quicksync_acquisition_mi355x::pcps_quicksync_acquisition_mi355x(const QuickSync_Acq_Conf& conf, int device)
    : acquisition_item_block_mi355x("pcps_quicksync_acquisition_mi355x", device, conf.fs_in, conf.doppler_max,
          conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_folding_factor(conf.folding_factor),
      d_max_dwells(conf.max_dwells),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code)),
      d_fft_size(conf.folding_factor ? static_cast<uint32_t>(conf.samples_per_code) / conf.folding_factor : 0),
      d_bit_transition_flag(conf.bit_transition_flag)
{
    d_set_state_activates = true;  // :199-221
    // with p = 1 the check of the delays reads past the item (delay + samples_per_code > L,
    // :396); beyond 100 it overruns complex_acumulator (:385)
    if (d_folding_factor < 2 || d_folding_factor > 16)
        throw std::invalid_argument("pcps_quicksync_acquisition_mi355x: folding_factor " +
                                    std::to_string(d_folding_factor) + " outside [2, 16]");
    // both folds would drop the last samples_per_code % p samples (:87, :146, :336)
    if (d_samples_per_code == 0 || d_samples_per_code % d_folding_factor != 0)
        throw std::invalid_argument("pcps_quicksync_acquisition_mi355x: " + std::to_string(d_samples_per_code) +
                                    " samples per code are no multiple of the folding factor " +
                                    std::to_string(d_folding_factor));
    // the block reads folding_factor * samples_per_code samples of every item (:310, :329)
    if (d_item_samples != d_folding_factor * d_samples_per_code)
        throw std::invalid_argument("pcps_quicksync_acquisition_mi355x: items of " + std::to_string(d_item_samples) +
                                    " samples, the search reads " + std::to_string(d_folding_factor * d_samples_per_code) +
                                    " (coherent_integration_time_ms must equal the folding factor)");
}

void pcps_quicksync_acquisition_mi355x::upload_code()
{
    if (!d_engine || d_code.empty()) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    if (gsdr_acq_set_quicksync_codes(d_engine, reinterpret_cast<const float*>(d_code.data()), &prn, 1) != GSDR_OK) fail();
}

// :135-157: the engine keeps the code unfolded and folds it for the grid
void pcps_quicksync_acquisition_mi355x::set_local_code(std::complex<float>* code)
{
    d_code.assign(code, code + d_samples_per_code);
    upload_code();
}

// :160-196
void pcps_quicksync_acquisition_mi355x::init()
{
    clear_synchro();
    if (d_doppler_step == 0) d_doppler_step = 250;  // :173-176
    create_engine(grid_conf(d_fft_size, d_samples_per_code), GSDR_WIPE_EXACT);
    if (gsdr_acq_set_quicksync(d_engine, d_folding_factor, d_samples_per_code) != GSDR_OK) fail();
    upload_code();
}

// the restart of :204-211 and :246-254
void pcps_quicksync_acquisition_mi355x::restart_counters() { d_well_count = 0; }

// general_work (:223-550)
int pcps_quicksync_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items)
{
    switch (d_state)
        {
        case 0:
            return idle_step(ninput_items);
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_quicksync_acquisition_mi355x: init() first");
                // :288-290
                d_input_power = 0.0;
                d_mag = 0.0;
                d_test_statistics = 0.0;
                // the reference advances the counter before the grid (:293, :417)
                const uint64_t first = d_sample_counter;
                d_sample_counter += static_cast<uint64_t>(d_item_samples);
                d_well_count++;
                const int rc = d_ring ? gsdr_acq_run_quicksync_stream(d_engine, d_ring, d_ring_origin + first, 1, first, &d_last)
                                      : gsdr_acq_run_quicksync(d_engine, in, 1, first, &d_last);
                if (rc != GSDR_OK) fail();
                d_input_power = d_last.input_power;
                // :370-423 over this item's rows: the record holds the last row that improved
                // d_mag and its check of the delays, the only one that survives the loop
                if (d_mag < d_last.mag)
                    {
                        d_mag = d_last.mag;
                        if (d_test_statistics < (d_mag / d_input_power) || !d_bit_transition_flag)
                            {
                                take_winner(d_last.acq_delay_samples, d_last.doppler_hz, d_last.samplestamp);
                                d_test_statistics = d_mag / d_input_power;  // :421
                            }
                    }
                // :443-467
                if (!d_bit_transition_flag)
                    {
                        if (d_test_statistics > d_threshold)
                            d_state = 2;  // Positive acquisition
                        else if (d_well_count == d_max_dwells)
                            d_state = 3;  // Negative acquisition
                    }
                else if (d_well_count == d_max_dwells)  // d_max_dwells = 2
                    d_state = d_test_statistics > d_threshold ? 2 : 3;
                return 1;
            }
        case 2:
        case 3:
            return terminal_step(d_state == 2, ninput_items);
        default:
            return 0;
        }
}
