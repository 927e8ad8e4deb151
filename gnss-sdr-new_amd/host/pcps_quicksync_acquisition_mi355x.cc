#include "pcps_quicksync_acquisition_mi355x.h"

#include <iostream>
#include <stdexcept>
#include <string>

namespace
{
[[noreturn]] void fail() { throw std::runtime_error(std::string("pcps_quicksync_acquisition_mi355x: ") + gsdr_last_error()); }
}  // namespace

// pcps_quicksync_acquisition_cc.cc:54-112
pcps_quicksync_acquisition_mi355x::pcps_quicksync_acquisition_mi355x(const QuickSync_Acq_Conf& conf, int device)
    : d_conf(conf),
      d_device(device),
      d_folding_factor(conf.folding_factor),
      d_doppler_max(conf.doppler_max),
      d_max_dwells(conf.max_dwells),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code)),
      d_fft_size(conf.folding_factor ? static_cast<uint32_t>(conf.samples_per_code) / conf.folding_factor : 0),
      d_item(conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_bit_transition_flag(conf.bit_transition_flag)
{
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
    if (d_item != d_folding_factor * d_samples_per_code)
        throw std::invalid_argument("pcps_quicksync_acquisition_mi355x: items of " + std::to_string(d_item) +
                                    " samples, the search reads " + std::to_string(d_folding_factor * d_samples_per_code) +
                                    " (coherent_integration_time_ms must equal the folding factor)");
}

pcps_quicksync_acquisition_mi355x::~pcps_quicksync_acquisition_mi355x() { gsdr_acq_destroy(d_engine); }

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
    d_gnss_synchro->Flag_valid_acquisition = false;
    d_gnss_synchro->Flag_valid_symbol_output = false;
    d_gnss_synchro->Flag_valid_pseudorange = false;
    d_gnss_synchro->Flag_valid_word = false;
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_mag = 0.0;
    d_input_power = 0.0;

    if (d_doppler_step == 0) d_doppler_step = 250;  // :173-176

    // Count the number of bins (:178-185)
    d_num_doppler_bins = 0;
    for (auto doppler = -static_cast<int32_t>(d_doppler_max); doppler <= static_cast<int32_t>(d_doppler_max);
         doppler += static_cast<int32_t>(d_doppler_step))
        d_num_doppler_bins++;

    gsdr_acq_destroy(d_engine);
    d_engine = nullptr;
    gsdr_acq_conf c{};
    c.fs_in = d_conf.fs_in;
    c.consumed_samples = d_fft_size;
    c.fft_size = d_fft_size;
    c.samples_per_code = static_cast<float>(d_samples_per_code);
    c.samples_per_chip = 1;  // the second-peak window: not used by a QuickSync run
    c.doppler_max = static_cast<int32_t>(d_doppler_max);
    c.doppler_step = d_doppler_step;
    c.num_doppler_bins = d_num_doppler_bins;
    c.pfa = 0.0F;
    c.max_dwells = 1;  // every dwell is a grid of its own
    c.item_type = GSDR_ITEM_GR_COMPLEX;
    c.max_prns = 1;
    c.max_blocks = 1;
    c.sampled_ms = 1;
    c.ms_per_code = 1;
    if (gsdr_acq_create(d_device, &c, &d_engine) != GSDR_OK)
        {
            d_engine = nullptr;
            fail();
        }
    if (gsdr_acq_set_wipeoff(d_engine, GSDR_WIPE_EXACT) != GSDR_OK) fail();
    if (gsdr_acq_set_quicksync(d_engine, d_folding_factor, d_samples_per_code) != GSDR_OK) fail();
    upload_code();
}

// the restart of :204-211 and :246-254
void pcps_quicksync_acquisition_mi355x::restart()
{
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_well_count = 0;
    d_mag = 0.0;
    d_input_power = 0.0;
    d_test_statistics = 0.0;
}

// :199-221
void pcps_quicksync_acquisition_mi355x::set_state(int32_t state)
{
    d_state = state;
    if (d_state == 1)
        {
            restart();
            d_active = true;
        }
    else if (d_state != 0)
        std::cerr << "State can only be set to 0 or 1\n";
}

void pcps_quicksync_acquisition_mi355x::set_ring(gsdr_stream* ring, uint64_t origin)
{
    d_ring = ring;
    d_ring_origin = origin;
}

// general_work (:223-550)
int pcps_quicksync_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items)
{
    int consumed = 0;
    switch (d_state)
        {
        case 0:
            if (d_active)
                {
                    restart();
                    d_state = 1;
                }
            d_sample_counter += static_cast<uint64_t>(d_item) * static_cast<uint64_t>(ninput_items);
            consumed = ninput_items;
            break;
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_quicksync_acquisition_mi355x: init() first");
                // :288-290
                d_input_power = 0.0;
                d_mag = 0.0;
                d_test_statistics = 0.0;
                // the engine stamps the item's first sample; the reference advances the counter
                // before the grid, so its stamp is the item's end (:293, :417)
                const uint64_t first = d_sample_counter;
                d_sample_counter += static_cast<uint64_t>(d_item);
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
                                d_gnss_synchro->Acq_delay_samples = d_last.acq_delay_samples;
                                d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_last.doppler_hz);
                                d_gnss_synchro->Acq_samplestamp_samples = d_last.samplestamp + d_item;
                                d_gnss_synchro->Acq_doppler_step = d_doppler_step;
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
                consumed = 1;
                break;
            }
        case 2:
        case 3:
            {
                const int message = d_state == 2 ? 1 : 2;
                d_active = false;
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(d_item) * static_cast<uint64_t>(ninput_items);
                consumed = ninput_items;
                if (d_events) d_events(message);
                break;
            }
        default:
            break;
        }
    return consumed;
}
