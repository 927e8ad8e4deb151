#include "acquisition_item_block_mi355x.h"

#include <iostream>
#include <stdexcept>

uint32_t acquisition_doppler_bins(uint32_t doppler_max, uint32_t doppler_step)
{
    uint32_t bins = 0;
    for (auto doppler = -static_cast<int32_t>(doppler_max); doppler <= static_cast<int32_t>(doppler_max);
         doppler += static_cast<int32_t>(doppler_step))
        bins++;
    return bins;
}

acquisition_item_block_mi355x::acquisition_item_block_mi355x(const char* name, int device, int64_t fs_in,
    uint32_t doppler_max, uint32_t item_samples)
    : d_name(name), d_device(device), d_fs_in(fs_in), d_doppler_max(doppler_max), d_item_samples(item_samples)
{
}

acquisition_item_block_mi355x::~acquisition_item_block_mi355x() { gsdr_acq_destroy(d_engine); }

void acquisition_item_block_mi355x::fail() const { throw std::runtime_error(d_name + ": " + gsdr_last_error()); }

void acquisition_item_block_mi355x::set_threshold(float threshold)
{
    d_threshold = threshold;
    if (d_threshold_on_engine && d_engine && gsdr_acq_set_threshold(d_engine, d_threshold) != GSDR_OK) fail();
}

void acquisition_item_block_mi355x::clear_synchro()
{
    d_gnss_synchro->Flag_valid_acquisition = false;
    d_gnss_synchro->Flag_valid_symbol_output = false;
    d_gnss_synchro->Flag_valid_pseudorange = false;
    d_gnss_synchro->Flag_valid_word = false;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_mag = 0.0;
    d_input_power = 0.0;
}

gsdr_acq_conf acquisition_item_block_mi355x::grid_conf(uint32_t fft_size, uint32_t samples_per_code)
{
    d_num_doppler_bins = acquisition_doppler_bins(d_doppler_max, d_doppler_step);
    gsdr_acq_conf c{};
    c.fs_in = d_fs_in;
    c.consumed_samples = fft_size;
    c.fft_size = fft_size;
    c.samples_per_code = static_cast<float>(samples_per_code);
    c.samples_per_chip = 1;  // the second-peak window: not used by these runs
    c.doppler_max = static_cast<int32_t>(d_doppler_max);
    c.doppler_step = d_doppler_step;
    c.num_doppler_bins = d_num_doppler_bins;
    c.pfa = 0.0F;
    c.max_dwells = 1;  // every item is a grid of its own; the dwells are the block's
    c.item_type = GSDR_ITEM_GR_COMPLEX;
    c.max_prns = 1;
    c.max_blocks = 1;
    c.sampled_ms = 1;
    c.ms_per_code = 1;
    return c;
}

void acquisition_item_block_mi355x::create_engine(const gsdr_acq_conf& conf, int wipeoff_mode)
{
    gsdr_acq_destroy(d_engine);
    d_engine = nullptr;
    if (gsdr_acq_create(d_device, &conf, &d_engine) != GSDR_OK)
        {
            d_engine = nullptr;
            fail();
        }
    if (gsdr_acq_set_wipeoff(d_engine, wipeoff_mode) != GSDR_OK) fail();
}

void acquisition_item_block_mi355x::restart()
{
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_mag = 0.0;
    d_input_power = 0.0;
    d_test_statistics = 0.0;
    restart_counters();
}

void acquisition_item_block_mi355x::set_state(int32_t state)
{
    d_state = state;
    if (d_state == 1)
        {
            restart();
            if (d_set_state_activates) d_active = true;
        }
    else if (d_state != 0)
        std::cerr << "State can only be set to 0 or 1\n";
}

void acquisition_item_block_mi355x::set_ring(gsdr_stream* ring, uint64_t origin)
{
    d_ring = ring;
    d_ring_origin = origin;
}

int acquisition_item_block_mi355x::idle_step(int ninput_items)
{
    if (d_active)
        {
            restart();
            d_state = 1;
        }
    d_sample_counter += static_cast<uint64_t>(d_item_samples) * static_cast<uint64_t>(ninput_items);
    return ninput_items;
}

int acquisition_item_block_mi355x::terminal_step(bool positive, int ninput_items, Gnss_Synchro* monitor_out,
    int* noutput_items)
{
    if (positive && monitor_out)
        {
            *monitor_out = *d_gnss_synchro;
            if (noutput_items) *noutput_items = 1;
        }
    d_active = false;
    d_state = 0;
    d_sample_counter += static_cast<uint64_t>(d_item_samples) * static_cast<uint64_t>(ninput_items);
    if (d_events) d_events(positive ? 1 : 2);
    return ninput_items;
}

void acquisition_item_block_mi355x::take_winner(double acq_delay_samples, int32_t doppler_hz, uint64_t item_first_sample)
{
    d_gnss_synchro->Acq_delay_samples = acq_delay_samples;
    d_gnss_synchro->Acq_doppler_hz = static_cast<double>(doppler_hz);
    d_gnss_synchro->Acq_samplestamp_samples = item_first_sample + d_item_samples;
    d_gnss_synchro->Acq_doppler_step = d_doppler_step;
}
