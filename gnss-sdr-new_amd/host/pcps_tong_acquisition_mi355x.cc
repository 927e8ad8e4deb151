#include "pcps_tong_acquisition_mi355x.h"

#include <algorithm>
#include <iostream>
#include <stdexcept>
#include <string>

namespace
{
[[noreturn]] void fail() { throw std::runtime_error(std::string("pcps_tong_acquisition_mi355x: ") + gsdr_last_error()); }
constexpr uint32_t kMaxBatch = 32;
}  // namespace

// pcps_tong_acquisition_cc.cc:68-119
pcps_tong_acquisition_mi355x::pcps_tong_acquisition_mi355x(const Tong_Acq_Conf& conf, int device)
    : d_conf(conf),
      d_device(device),
      d_doppler_max(conf.doppler_max),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code)),
      d_fft_size(conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_tong_init_val(conf.tong_init_val),
      d_tong_max_val(conf.tong_max_val),
      d_tong_max_dwells(conf.tong_max_dwells),
      d_tong_count(conf.tong_init_val),
      d_batch(std::max(1U, std::min(conf.tong_max_dwells, kMaxBatch))),
      d_enable_monitor_output(conf.enable_monitor_output)
{
    // d_tong_count is unsigned: from 0 the first miss wraps it (:362); at or above
    // tong_max_val it never meets the '==' of :355
    if (d_tong_init_val < 1 || d_tong_init_val >= d_tong_max_val)
        throw std::invalid_argument("pcps_tong_acquisition_mi355x: need 1 <= tong_init_val (" +
                                    std::to_string(d_tong_init_val) + ") < tong_max_val (" +
                                    std::to_string(d_tong_max_val) + ")");
    if (d_tong_max_dwells < 1) throw std::invalid_argument("pcps_tong_acquisition_mi355x: tong_max_dwells must be >= 1");
    if (d_fft_size == 0 || d_samples_per_code == 0)
        throw std::invalid_argument("pcps_tong_acquisition_mi355x: empty items or code");
}

pcps_tong_acquisition_mi355x::~pcps_tong_acquisition_mi355x() { gsdr_acq_destroy(d_engine); }

void pcps_tong_acquisition_mi355x::upload_code()
{
    if (!d_engine || d_code.empty()) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    if (gsdr_acq_set_local_codes(d_engine, reinterpret_cast<const float*>(d_code.data()), &prn, 1) != GSDR_OK) fail();
}

// :142-150
void pcps_tong_acquisition_mi355x::set_local_code(std::complex<float>* code)
{
    d_code.assign(code, code + d_fft_size);
    upload_code();
}

void pcps_tong_acquisition_mi355x::set_threshold(float threshold)
{
    d_threshold = threshold;
    if (d_engine && gsdr_acq_set_threshold(d_engine, d_threshold) != GSDR_OK) fail();
}

// :153-185
void pcps_tong_acquisition_mi355x::init()
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

    // the reference's loop over the bins does not end with a zero step (:168-173)
    if (d_doppler_step == 0) throw std::invalid_argument("pcps_tong_acquisition_mi355x: set_doppler_step before init");

    // Count the number of bins (:166-173)
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
    c.samples_per_chip = 1;  // the second-peak window: not used by a Tong run
    c.doppler_max = static_cast<int32_t>(d_doppler_max);
    c.doppler_step = d_doppler_step;
    c.num_doppler_bins = d_num_doppler_bins;
    c.pfa = 0.0F;
    c.max_dwells = 1;  // the dwells are the Tong sequence's
    c.item_type = GSDR_ITEM_GR_COMPLEX;
    c.max_prns = 1;
    c.max_blocks = d_batch;
    c.sampled_ms = 1;
    c.ms_per_code = 1;
    if (gsdr_acq_create(d_device, &c, &d_engine) != GSDR_OK)
        {
            d_engine = nullptr;
            fail();
        }
    if (gsdr_acq_set_wipeoff(d_engine, GSDR_WIPE_EXACT) != GSDR_OK) fail();
    if (gsdr_acq_set_tong(d_engine, d_tong_init_val, d_tong_max_val, d_tong_max_dwells) != GSDR_OK) fail();
    if (gsdr_acq_set_threshold(d_engine, d_threshold) != GSDR_OK) fail();
    d_records.assign(d_batch, gsdr_acq_tong_result{});
    upload_code();
}

// the restart of :193-209 and :233-250; the grid is zeroed by the engine's reset
void pcps_tong_acquisition_mi355x::restart()
{
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_dwell_count = 0;
    d_tong_count = d_tong_init_val;
    d_mag = 0.0;
    d_input_power = 0.0;
    d_test_statistics = 0.0;
    if (d_engine && gsdr_acq_tong_reset(d_engine, nullptr, 0) != GSDR_OK) fail();
}

// :188-218
void pcps_tong_acquisition_mi355x::set_state(int32_t state)
{
    d_state = state;
    if (d_state == 1)
        restart();
    else if (d_state != 0)
        std::cerr << "State can only be set to 0 or 1\n";
}

void pcps_tong_acquisition_mi355x::set_ring(gsdr_stream* ring, uint64_t origin)
{
    d_ring = ring;
    d_ring_origin = origin;
}

// general_work (:221-440)
int pcps_tong_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items, Gnss_Synchro* monitor_out,
    int* noutput_items)
{
    int consumed = 0;
    if (noutput_items) *noutput_items = 0;
    switch (d_state)
        {
        case 0:
            if (d_active)
                {
                    restart();
                    d_state = 1;
                }
            d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(ninput_items);
            consumed = ninput_items;
            break;
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_tong_acquisition_mi355x: init() first");
                if (ninput_items < 1) break;
                // as many state-1 calls of the reference as items offered, in one engine call:
                // no sequence goes beyond tong_max_dwells items
                const uint32_t left = d_tong_max_dwells > d_dwell_count ? d_tong_max_dwells - d_dwell_count : 1U;
                const uint32_t n = std::min({static_cast<uint32_t>(ninput_items), d_batch, left});
                const uint64_t first = d_sample_counter;
                const int rc = d_ring ? gsdr_acq_run_tong_stream(d_engine, d_ring, d_ring_origin + first, n, first, d_records.data())
                                      : gsdr_acq_run_tong(d_engine, in, n, first, d_records.data());
                if (rc != GSDR_OK) fail();
                // up to and including the first item that ends the sequence
                uint32_t used = 0;
                while (used < n && d_records[used].state == GSDR_TONG_RUNNING) ++used;
                if (used < n) ++used;
                d_last = d_records[used - 1];
                // the engine stamps the item's first sample; the reference advances the counter
                // before the grid, so its stamp is the item's end (:272, :330)
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * used;
                d_dwell_count = d_last.dwell_count;
                d_tong_count = d_last.tong_count;
                d_input_power = d_last.input_power;
                d_mag = 0.0;
                if (d_mag < d_last.mag)  // :325
                    {
                        d_mag = d_last.mag;
                        d_gnss_synchro->Acq_delay_samples = d_last.acq_delay_samples;
                        d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_last.doppler_hz);
                        d_gnss_synchro->Acq_samplestamp_samples = d_last.samplestamp + d_fft_size;
                        d_gnss_synchro->Acq_doppler_step = d_doppler_step;
                    }
                d_test_statistics = d_mag;  // :350
                if (d_last.state == GSDR_TONG_POSITIVE)
                    d_state = 2;
                else if (d_last.state == GSDR_TONG_NEGATIVE)
                    d_state = 3;
                consumed = static_cast<int>(used);
                break;
            }
        case 2:
        case 3:
            {
                const int message = d_state == 2 ? 1 : 2;
                // :401-408: the monitor output of a positive acquisition
                if (d_state == 2 && d_enable_monitor_output && monitor_out)
                    {
                        *monitor_out = *d_gnss_synchro;
                        if (noutput_items) *noutput_items = 1;
                    }
                d_active = false;
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(ninput_items);
                consumed = ninput_items;
                if (d_events) d_events(message);
                break;
            }
        default:
            break;
        }
    return consumed;
}
