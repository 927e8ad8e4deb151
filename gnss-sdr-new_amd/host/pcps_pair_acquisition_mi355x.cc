#include "pcps_pair_acquisition_mi355x.h"

#include <stdexcept>

// pcps_cccwsr_acquisition_cc.cc:50-103, galileo_pcps_8ms_acquisition_cc.cc:47-92
pcps_pair_acquisition_mi355x::pcps_pair_acquisition_mi355x(const Pair_Acq_Conf& conf, int device)
    : acquisition_item_block_mi355x("pcps_pair_acquisition_mi355x", device, conf.fs_in, conf.doppler_max,
          conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_conf(conf),
      d_max_dwells(conf.max_dwells),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code))
{
    // the 8 ms block's code B negates samples [samples_per_code, 2 samples_per_code) of an
    // fft_size buffer (:126-129): with one code period per item the reference writes past
    // the buffer's end
    if (conf.policy == Pair_Acq_Conf::PCPS_8MS && d_item_samples < 2 * d_samples_per_code)
        throw std::invalid_argument(
            "pcps_pair_acquisition_mi355x: the 8 ms acquisition needs at least two code periods per item "
            "(coherent_integration_time_ms >= 8)");
}

void pcps_pair_acquisition_mi355x::upload_codes()
{
    if (!d_engine || d_first.empty()) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    const int kind = d_conf.policy == Pair_Acq_Conf::CCCWSR ? GSDR_ACQ_PAIR_SUM_DIFF_J : GSDR_ACQ_PAIR_AS_IS;
    if (gsdr_acq_set_code_pairs(d_engine, kind, reinterpret_cast<const float*>(d_first.data()),
            reinterpret_cast<const float*>(d_second.data()), &prn, 1) != GSDR_OK)
        fail();
}

// :126-144: the reference's own two arguments; the engine forms data -+ j pilot
void pcps_pair_acquisition_mi355x::set_local_code(std::complex<float>* code_data, std::complex<float>* code_pilot)
{
    d_first.assign(code_data, code_data + d_item_samples);
    d_second.assign(code_pilot, code_pilot + d_item_samples);
    upload_codes();
}

// galileo_pcps_8ms_acquisition_cc.cc:114-135: code A as given; code B the same buffer with
// the second code period inverted (only that one, whatever the item's length)
void pcps_pair_acquisition_mi355x::set_local_code(std::complex<float>* code)
{
    d_first.assign(code, code + d_item_samples);
    d_second = d_first;
    for (uint32_t i = d_samples_per_code; i < 2 * d_samples_per_code; ++i) d_second[i] = -d_second[i];
    upload_codes();
}

// :147-177
void pcps_pair_acquisition_mi355x::init()
{
    clear_synchro();
    // Count the number of bins (:160-166)
    if (d_doppler_step == 0) throw std::invalid_argument("pcps_pair_acquisition_mi355x: set_doppler_step before init");
    gsdr_acq_conf c = grid_conf(d_item_samples, d_samples_per_code);
    c.max_prns = 2;
    c.sampled_ms = d_conf.sampled_ms;
    c.ms_per_code = d_conf.sampled_ms;
    create_engine(c, d_conf.wipeoff_mode);
    upload_codes();
}

// the restart of :191-200 and :217-228
void pcps_pair_acquisition_mi355x::restart_counters() { d_well_count = 0; }

// general_work (:205-436)
int pcps_pair_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items)
{
    switch (d_state)
        {
        case 0:
            return idle_step(ninput_items);
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_pair_acquisition_mi355x: init() first");
                if (d_conf.policy == Pair_Acq_Conf::PCPS_8MS)
                    {
                        // galileo_pcps_8ms_acquisition_cc.cc:238-239
                        d_input_power = 0.0;
                        d_mag = 0.0;
                    }
                // the reference advances the counter before the grid (:241, :339)
                const uint64_t first = d_sample_counter;
                d_sample_counter += static_cast<uint64_t>(d_item_samples);
                d_well_count++;
                const int rc = d_ring ? gsdr_acq_run_pairs_stream(d_engine, d_ring, d_ring_origin + first, 1, first, &d_last)
                                      : gsdr_acq_run_pairs(d_engine, in, 1, first, &d_last);
                if (rc != GSDR_OK) fail();
                d_input_power = d_last.input_power;
                // :334-341 over this item's rows: its grid maximum against what d_mag holds
                if (d_mag < d_last.mag)
                    {
                        d_mag = d_last.mag;
                        take_winner(d_last.acq_delay_samples, d_last.doppler_hz, d_last.samplestamp);
                    }
                d_test_statistics = d_mag / d_input_power;  // :360
                if (d_test_statistics > d_threshold)
                    d_state = 2;  // Positive acquisition
                else if (d_well_count == d_max_dwells)
                    d_state = 3;  // Negative acquisition
                return 1;
            }
        case 2:
        case 3:
            return terminal_step(d_state == 2, ninput_items);
        default:
            return 0;
        }
}
