#include "pcps_pair_acquisition_mi355x.h"

#include <iostream>
#include <stdexcept>

namespace
{
[[noreturn]] void fail() { throw std::runtime_error(std::string("pcps_pair_acquisition_mi355x: ") + gsdr_last_error()); }
}  // namespace

// pcps_cccwsr_acquisition_cc.cc:50-103, galileo_pcps_8ms_acquisition_cc.cc:47-92
pcps_pair_acquisition_mi355x::pcps_pair_acquisition_mi355x(const Pair_Acq_Conf& conf, int device)
    : d_conf(conf),
      d_device(device),
      d_doppler_max(conf.doppler_max),
      d_max_dwells(conf.max_dwells),
      d_fft_size(conf.sampled_ms * static_cast<uint32_t>(conf.samples_per_ms)),
      d_samples_per_code(static_cast<uint32_t>(conf.samples_per_code))
{
    // the 8 ms block's code B negates samples [samples_per_code, 2 samples_per_code) of an
    // fft_size buffer (:126-129): with one code period per item the reference writes past
    // the buffer's end
    if (conf.policy == Pair_Acq_Conf::PCPS_8MS && d_fft_size < 2 * d_samples_per_code)
        throw std::invalid_argument(
            "pcps_pair_acquisition_mi355x: the 8 ms acquisition needs at least two code periods per item "
            "(coherent_integration_time_ms >= 8)");
}

pcps_pair_acquisition_mi355x::~pcps_pair_acquisition_mi355x() { gsdr_acq_destroy(d_engine); }

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
    d_first.assign(code_data, code_data + d_fft_size);
    d_second.assign(code_pilot, code_pilot + d_fft_size);
    upload_codes();
}

// galileo_pcps_8ms_acquisition_cc.cc:114-135: code A as given; code B the same buffer with
// the second code period inverted (only that one, whatever the item's length)
void pcps_pair_acquisition_mi355x::set_local_code(std::complex<float>* code)
{
    d_first.assign(code, code + d_fft_size);
    d_second = d_first;
    for (uint32_t i = d_samples_per_code; i < 2 * d_samples_per_code; ++i) d_second[i] = -d_second[i];
    upload_codes();
}

// :147-177
void pcps_pair_acquisition_mi355x::init()
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

    // Count the number of bins (:160-166)
    if (d_doppler_step == 0) throw std::invalid_argument("pcps_pair_acquisition_mi355x: set_doppler_step before init");
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
    c.samples_per_chip = 1;  // the second-peak window: not used by a pair run
    c.doppler_max = static_cast<int32_t>(d_doppler_max);
    c.doppler_step = d_doppler_step;
    c.num_doppler_bins = d_num_doppler_bins;
    c.pfa = 0.0F;
    c.max_dwells = 1;  // every dwell is a grid of its own
    c.item_type = GSDR_ITEM_GR_COMPLEX;
    c.max_prns = 2;
    c.max_blocks = 1;
    c.sampled_ms = d_conf.sampled_ms;
    c.ms_per_code = d_conf.sampled_ms;
    if (gsdr_acq_create(d_device, &c, &d_engine) != GSDR_OK)
        {
            d_engine = nullptr;
            fail();
        }
    if (gsdr_acq_set_wipeoff(d_engine, d_conf.wipeoff_mode) != GSDR_OK) fail();
    upload_codes();
}

// the restart of :191-200 and :217-228
void pcps_pair_acquisition_mi355x::restart()
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

// :180-202
void pcps_pair_acquisition_mi355x::set_state(int32_t state)
{
    d_state = state;
    if (d_state == 1)
        restart();
    else if (d_state != 0)
        std::cerr << "State can only be set to 0 or 1\n";
}

void pcps_pair_acquisition_mi355x::set_ring(gsdr_stream* ring, uint64_t origin)
{
    d_ring = ring;
    d_ring_origin = origin;
}

// general_work (:205-436)
int pcps_pair_acquisition_mi355x::work(const std::complex<float>* in, int ninput_items)
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
            d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(ninput_items);
            consumed = ninput_items;
            break;
        case 1:
            {
                if (!d_engine) throw std::runtime_error("pcps_pair_acquisition_mi355x: init() first");
                if (d_conf.policy == Pair_Acq_Conf::PCPS_8MS)
                    {
                        // galileo_pcps_8ms_acquisition_cc.cc:238-239
                        d_input_power = 0.0;
                        d_mag = 0.0;
                    }
                // the engine stamps the item's first sample; the reference advances the
                // counter before the grid, so its stamp is the item's end (:241, :339)
                const uint64_t first = d_sample_counter;
                d_sample_counter += static_cast<uint64_t>(d_fft_size);
                d_well_count++;
                const int rc = d_ring ? gsdr_acq_run_pairs_stream(d_engine, d_ring, d_ring_origin + first, 1, first, &d_last)
                                      : gsdr_acq_run_pairs(d_engine, in, 1, first, &d_last);
                if (rc != GSDR_OK) fail();
                d_input_power = d_last.input_power;
                // :334-341 over this item's rows: its grid maximum against what d_mag holds
                if (d_mag < d_last.mag)
                    {
                        d_mag = d_last.mag;
                        d_gnss_synchro->Acq_delay_samples = d_last.acq_delay_samples;
                        d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_last.doppler_hz);
                        d_gnss_synchro->Acq_samplestamp_samples = d_last.samplestamp + d_fft_size;
                        d_gnss_synchro->Acq_doppler_step = d_doppler_step;
                    }
                d_test_statistics = d_mag / d_input_power;  // :360
                if (d_test_statistics > d_threshold)
                    d_state = 2;  // Positive acquisition
                else if (d_well_count == d_max_dwells)
                    d_state = 3;  // Negative acquisition
                consumed = 1;
                break;
            }
        case 2:
        case 3:
            {
                const int message = d_state == 2 ? 1 : 2;
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
