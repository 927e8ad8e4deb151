#include "galileo_e5a_noncoherent_iq_acquisition_caf_block_mi355x.h"

#include <algorithm>
#include <stdexcept>

namespace
{
constexpr uint32_t kMaxBatch = 32;
}  // namespace

// galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:55-137
galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::galileo_e5a_noncoherentIQ_acquisition_caf_mi355x(
    const E5a_Iq_Caf_Acq_Conf& conf, int device)
    : acquisition_item_block_mi355x("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x", device, conf.fs_in,
          conf.doppler_max, conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_CAF_window_hz(conf.CAF_window_hz),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code)),
      d_sampled_ms(conf.Zero_padding > 0 ? 1U : conf.sampled_ms),
      d_max_dwells(conf.max_dwells),
      d_batch(std::max(1U, std::min(conf.max_dwells, kMaxBatch))),
      d_bit_transition_flag(conf.bit_transition_flag),
      d_both_signal_components(conf.both_signal_components),
      d_enable_monitor_output(conf.enable_monitor_output)
{
    d_doppler_step = 250;  // :88
    // d_well_count == d_max_dwells (:686) is never met from 1 upwards
    if (d_max_dwells < 1)
        throw std::invalid_argument("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x: max_dwells must be >= 1");
    if (d_item_samples == 0 || d_samples_per_code == 0 || d_samples_per_code > d_item_samples)
        throw std::invalid_argument("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x: empty items or code");
    if (d_sampled_ms < 1 || d_sampled_ms > 3)
        throw std::invalid_argument("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x: 1 to 3 ms of coherent integration");
}

void galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::upload_code()
{
    if (!d_engine || d_code_i.empty()) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    if (gsdr_acq_set_iq_codes(d_engine, reinterpret_cast<const float*>(d_code_i.data()),
            d_both_signal_components ? reinterpret_cast<const float*>(d_code_q.data()) : nullptr, &prn, 1) != GSDR_OK)
        fail();
}

// :160-208
void galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::set_local_code(std::complex<float>* codeI, std::complex<float>* codeQ)
{
    d_code_i.assign(codeI, codeI + d_item_samples);
    if (d_both_signal_components) d_code_q.assign(codeQ, codeQ + d_item_samples);
    upload_code();
}

// :211-255
void galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::init()
{
    clear_synchro();
    // the reference's loop over the bins does not end with a zero step (:227-232)
    if (d_doppler_step == 0)
        throw std::invalid_argument("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x: doppler_step 0");
    gsdr_acq_conf c = grid_conf(d_item_samples, d_samples_per_code);
    c.max_prns = (d_sampled_ms > 1 ? 2U : 1U) * (d_both_signal_components ? 2U : 1U);
    c.max_blocks = d_batch;
    create_engine(c, GSDR_WIPE_EXACT);
    // refuses the windows with which :605 divides by zero or :609-667 leave their vectors
    if (gsdr_acq_set_iq_caf(d_engine, d_samples_per_code, d_sampled_ms, d_both_signal_components ? 1 : 0,
            d_CAF_window_hz) != GSDR_OK)
        fail();
    d_records.assign(d_batch, gsdr_acq_iq_caf_result{});
    upload_code();
}

// the restart of :261-271 and :310-321
void galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::restart_counters() { d_well_count = 0; }

// general_work (:282-764)
int galileo_e5a_noncoherentIQ_acquisition_caf_mi355x::work(const std::complex<float>* in, int ninput_items,
    Gnss_Synchro* monitor_out, int* noutput_items)
{
    if (noutput_items) *noutput_items = 0;
    switch (d_state)
        {
        case 0:
            return idle_step(ninput_items);
        case 1:
            {
                if (!d_engine) throw std::runtime_error("galileo_e5a_noncoherentIQ_acquisition_caf_mi355x: init() first");
                if (ninput_items < 1) return 0;
                // as many dwells of the reference as items offered, in one engine call: no attempt
                // goes beyond max_dwells items
                const uint32_t left = d_max_dwells > d_well_count ? d_max_dwells - d_well_count : 1U;
                const uint32_t n = std::min({static_cast<uint32_t>(ninput_items), d_batch, left});
                const uint64_t first = d_sample_counter;
                const int rc = d_ring ? gsdr_acq_run_iq_caf_stream(d_engine, d_ring, d_ring_origin + first, n, first,
                                            d_records.data())
                                      : gsdr_acq_run_iq_caf(d_engine, in, n, first, d_records.data());
                if (rc != GSDR_OK) fail();
                for (uint32_t k = 0; k < n; ++k)
                    {
                        d_last = d_records[k];
                        // the reference has counted the item before it runs the grid (:359, :563)
                        d_sample_counter += d_item_samples;
                        d_input_power = d_last.input_power;
                        d_mag = 0.0;
                        d_well_count++;
                        // the rows' maxima ascend to the winner's and :559 is tested at each step:
                        // the last row that passes is the winner, or none does
                        if (d_mag < d_last.mag)
                            {
                                d_mag = d_last.mag;
                                if (d_test_statistics < (d_mag / d_input_power) || !d_bit_transition_flag)
                                    {
                                        take_winner(d_last.acq_delay_samples, d_last.doppler_hz, d_last.samplestamp);
                                        d_test_statistics = d_mag / d_input_power;
                                    }
                            }
                        // :670-672
                        if (d_CAF_window_hz > 0) d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_last.caf_doppler_hz);
                    }
                // :686-700 (n never passes the dwell that decides)
                if (d_well_count == d_max_dwells) d_state = d_test_statistics > d_threshold ? 3 : 4;
                return static_cast<int>(n);
            }
        case 3:
        case 4:
            // :728-735: the monitor output of a positive acquisition
            return terminal_step(d_state == 3, ninput_items, d_enable_monitor_output ? monitor_out : nullptr, noutput_items);
        default:
            return 0;
        }
}
