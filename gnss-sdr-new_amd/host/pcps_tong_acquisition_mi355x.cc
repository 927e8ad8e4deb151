#include "pcps_tong_acquisition_mi355x.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace
{
constexpr uint32_t kMaxBatch = 32;
}  // namespace

// pcps_tong_acquisition_cc.cc:68-119
pcps_tong_acquisition_mi355x::pcps_tong_acquisition_mi355x(const Tong_Acq_Conf& conf, int device)
    : acquisition_item_block_mi355x("pcps_tong_acquisition_mi355x", device, conf.fs_in, conf.doppler_max,
          conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code)),
      d_tong_init_val(conf.tong_init_val),
      d_tong_max_val(conf.tong_max_val),
      d_tong_max_dwells(conf.tong_max_dwells),
      d_tong_count(conf.tong_init_val),
      d_batch(std::max(1U, std::min(conf.tong_max_dwells, kMaxBatch))),
      d_enable_monitor_output(conf.enable_monitor_output)
{
    d_threshold_on_engine = true;
    // d_tong_count is unsigned: from 0 the first miss wraps it (:362); at or above
    // tong_max_val it never meets the '==' of :355
    if (d_tong_init_val < 1 || d_tong_init_val >= d_tong_max_val)
        throw std::invalid_argument("pcps_tong_acquisition_mi355x: need 1 <= tong_init_val (" +
                                    std::to_string(d_tong_init_val) + ") < tong_max_val (" +
                                    std::to_string(d_tong_max_val) + ")");
    if (d_tong_max_dwells < 1) throw std::invalid_argument("pcps_tong_acquisition_mi355x: tong_max_dwells must be >= 1");
    if (d_item_samples == 0 || d_samples_per_code == 0)
        throw std::invalid_argument("pcps_tong_acquisition_mi355x: empty items or code");
}

void pcps_tong_acquisition_mi355x::upload_code()
{
    if (!d_engine || d_code.empty()) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    if (gsdr_acq_set_local_codes(d_engine, reinterpret_cast<const float*>(d_code.data()), &prn, 1) != GSDR_OK) fail();
}

// :142-150
void pcps_tong_acquisition_mi355x::set_local_code(std::complex<float>* code)
{
    d_code.assign(code, code + d_item_samples);
    upload_code();
}

// :153-185
void pcps_tong_acquisition_mi355x::init()
{
    clear_synchro();
    // the reference's loop over the bins does not end with a zero step (:168-173)
    if (d_doppler_step == 0) throw std::invalid_argument("pcps_tong_acquisition_mi355x: set_doppler_step before init");
    gsdr_acq_conf c = grid_conf(d_item_samples, d_samples_per_code);
    c.max_blocks = d_batch;
    create_engine(c, GSDR_WIPE_EXACT);
    if (gsdr_acq_set_tong(d_engine, d_tong_init_val, d_tong_max_val, d_tong_max_dwells) != GSDR_OK) fail();
    if (gsdr_acq_set_threshold(d_engine, d_threshold) != GSDR_OK) fail();
    d_records.assign(d_batch, gsdr_acq_tong_result{});
    upload_code();
}

// the restart of :193-209 and :233-250; the grid is zeroed by the engine's reset
void pcps_tong_acquisition_mi355x::restart_counters()
{
    d_dwell_count = 0;
    d_tong_count = d_tong_init_val;
    if (d_engine && gsdr_acq_tong_reset(d_engine, nullptr, 0) != GSDR_OK) fail();
}

// general_work (:221-440)
int pcps_tong_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items, Gnss_Synchro* monitor_out,
    int* noutput_items)
{
    if (noutput_items) *noutput_items = 0;
    switch (d_state)
        {
        case 0:
            return idle_step(ninput_items);
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_tong_acquisition_mi355x: init() first");
                if (ninput_items < 1) return 0;
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
                // the reference advances the counter before the grid (:272, :330)
                d_sample_counter += static_cast<uint64_t>(d_item_samples) * used;
                d_dwell_count = d_last.dwell_count;
                d_tong_count = d_last.tong_count;
                d_input_power = d_last.input_power;
                d_mag = 0.0;
                if (d_mag < d_last.mag)  // :325
                    {
                        d_mag = d_last.mag;
                        take_winner(d_last.acq_delay_samples, d_last.doppler_hz, d_last.samplestamp);
                    }
                d_test_statistics = d_mag;  // :350
                if (d_last.state == GSDR_TONG_POSITIVE)
                    d_state = 2;
                else if (d_last.state == GSDR_TONG_NEGATIVE)
                    d_state = 3;
                return static_cast<int>(used);
            }
        case 2:
        case 3:
            // :401-408: the monitor output of a positive acquisition
            return terminal_step(d_state == 2, ninput_items, d_enable_monitor_output ? monitor_out : nullptr, noutput_items);
        default:
            return 0;
        }
}
