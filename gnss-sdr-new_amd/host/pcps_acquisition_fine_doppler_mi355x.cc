#include "pcps_acquisition_fine_doppler_mi355x.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <stdexcept>

#include "mat5_writer.h"

namespace
{
constexpr double GPS_L1_CA_CHIP_PERIOD_S = 9.7752e-07;  // GPS_L1_CA.h:38
}

// pcps_acquisition_fine_doppler_cc.cc:43-110
pcps_acquisition_fine_doppler_mi355x::pcps_acquisition_fine_doppler_mi355x(const Acq_Conf& conf, int device)
    : acq_parameters(conf),
      d_device(device),
      d_dump_filename(conf.dump_filename),
      d_fs_in(conf.fs_in),
      d_samples_per_ms(static_cast<int>(conf.samples_per_ms)),
      d_max_dwells(static_cast<int>(conf.max_dwells)),
      d_config_doppler_max(conf.doppler_max),
      d_fft_size(d_samples_per_ms),
      d_dump(conf.dump)
{
    // d_10_ms_buffer holds the dwell blocks followed by what state 3 collects (:73: 50 ms;
    // more dwells than that would overrun the reference's buffer)
    d_10_ms_buffer.resize(static_cast<size_t>(std::max(50, d_max_dwells)) * d_samples_per_ms);
    if (d_dump)
        {
            // :79-109: <path>/<name without extension>
            std::string dump_path;
            const auto slash = d_dump_filename.find_last_of('/');
            if (slash != std::string::npos)
                {
                    dump_path = d_dump_filename.substr(0, slash);
                    d_dump_filename = d_dump_filename.substr(slash + 1);
                }
            else
                dump_path = ".";
            if (d_dump_filename.empty()) d_dump_filename = "acquisition";
            if (d_dump_filename.substr(1).find_last_of('.') != std::string::npos)
                d_dump_filename = d_dump_filename.substr(0, d_dump_filename.find_last_of('.'));
            d_dump_filename = dump_path + "/" + d_dump_filename;
            std::error_code ec;
            std::filesystem::create_directories(dump_path, ec);
            if (ec)
                {
                    std::cerr << "GNSS-SDR cannot create dump file for the Acquisition block. Wrong permissions?\n";
                    d_dump = false;
                }
        }
}

pcps_acquisition_fine_doppler_mi355x::~pcps_acquisition_fine_doppler_mi355x() { gsdr_acq_destroy(d_engine); }

// set_doppler_step (:129-144): the grid has floor(|2 doppler_max| / doppler_step) rows, one
// fewer than pcps_acquisition's ceil over the closed range; row i searches
// doppler_step * i - doppler_max (:202).
void pcps_acquisition_fine_doppler_mi355x::set_doppler_step(uint32_t doppler_step)
{
    d_doppler_step = doppler_step;
    d_num_doppler_points = static_cast<int>(std::floor(std::abs(2 * d_config_doppler_max) / d_doppler_step));
    gsdr_acq_destroy(d_engine);
    d_engine = nullptr;
    gsdr_acq_conf c{};
    c.fs_in = d_fs_in;
    c.consumed_samples = static_cast<uint32_t>(d_fft_size);
    c.fft_size = 0;
    c.samples_per_code = static_cast<float>(d_fft_size);
    // compute_CAF's exclusion half-width (:242)
    c.samples_per_chip = static_cast<uint32_t>(std::ceil(GPS_L1_CA_CHIP_PERIOD_S * static_cast<float>(d_fs_in)));
    c.doppler_max = d_config_doppler_max;
    c.doppler_step = d_doppler_step;
    c.num_doppler_bins = static_cast<uint32_t>(d_num_doppler_points);
    c.pfa = 0.0F;  // first / second peak (:241-273)
    c.max_dwells = static_cast<uint32_t>(d_max_dwells);
    c.item_type = GSDR_ITEM_GR_COMPLEX;
    c.max_prns = 1;
    c.max_blocks = 1;
    c.sampled_ms = 1;
    c.ms_per_code = 1;
    if (gsdr_acq_create(d_device, &c, &d_engine) != GSDR_OK)
        {
            d_engine = nullptr;
            throw std::runtime_error(std::string("pcps_acquisition_fine_doppler_mi355x: ") + gsdr_last_error());
        }
    if (gsdr_acq_set_wipeoff(d_engine, acq_parameters.wipeoff_mode()) != GSDR_OK)
        throw std::runtime_error(std::string("pcps_acquisition_fine_doppler_mi355x: ") + gsdr_last_error());
    if (d_dump) d_grid.assign(static_cast<size_t>(d_fft_size) * d_num_doppler_points, 0.0F);
    if (!d_code.empty())
        {
            const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
            gsdr_acq_set_local_codes(d_engine, reinterpret_cast<const float*>(d_code.data()), &prn, 1);
        }
}

// set_local_code (:147-153); the row is kept: estimate_Doppler's replica (:363, the same
// gps_l1_ca_code_gen_complex_sampled output the adapter passes here) is wiped off with it
void pcps_acquisition_fine_doppler_mi355x::set_local_code(std::complex<float>* code)
{
    d_code.assign(code, code + d_fft_size);
    if (!d_engine) return;
    const uint32_t prn = d_gnss_synchro ? d_gnss_synchro->PRN : 0;
    if (gsdr_acq_set_local_codes(d_engine, reinterpret_cast<const float*>(d_code.data()), &prn, 1) != GSDR_OK)
        throw std::runtime_error(std::string("pcps_acquisition_fine_doppler_mi355x: ") + gsdr_last_error());
}

// :156-167
void pcps_acquisition_fine_doppler_mi355x::init()
{
    d_gnss_synchro->Flag_valid_acquisition = false;
    d_gnss_synchro->Flag_valid_symbol_output = false;
    d_gnss_synchro->Flag_valid_pseudorange = false;
    d_gnss_synchro->Flag_valid_word = false;
    d_gnss_synchro->Acq_doppler_step = 0U;
    d_gnss_synchro->Acq_delay_samples = 0.0;
    d_gnss_synchro->Acq_doppler_hz = 0.0;
    d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
    d_state = 0;
}

// :180-191: dwell 0 of gsdr_acq_run_dwell restarts the device grid
void pcps_acquisition_fine_doppler_mi355x::reset_grid()
{
    d_well_count = 0;
    if (d_dump) std::fill(d_grid.begin(), d_grid.end(), 0.0F);
}

bool pcps_acquisition_fine_doppler_mi355x::start()
{
    d_sample_counter = 0ULL;
    return true;
}

// :430-453
void pcps_acquisition_fine_doppler_mi355x::set_state(int state)
{
    d_state = state;
    if (d_state == 1)
        {
            d_gnss_synchro->Acq_delay_samples = 0.0;
            d_gnss_synchro->Acq_doppler_hz = 0.0;
            d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
            d_gnss_synchro->Acq_doppler_step = 0U;
            d_well_count = 0;
            d_test_statistics = 0.0;
            d_active = true;
            reset_grid();
            d_window_first = d_sample_counter;
        }
    else if (d_state != 0)
        std::cerr << "State can only be set to 0 or 1\n";
}

void pcps_acquisition_fine_doppler_mi355x::set_ring(gsdr_stream* ring, uint64_t origin)
{
    d_ring = ring;
    d_ring_origin = origin;
}

// compute_CAF (:213-282) on the grid accumulated by the max_dwells run_dwell calls: the last
// call's record is the first / second peak statistic of that grid, with the exclusion and
// the one-sided wrap of pcps_acquisition.cc:584-604, which are this block's too (:241-266).
float pcps_acquisition_fine_doppler_mi355x::compute_CAF()
{
    d_test_statistics = d_coarse.test_statistic;
    d_gnss_synchro->Acq_delay_samples = static_cast<double>(d_coarse.code_phase);  // the raw row index (:276)
    d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_coarse.doppler_hz);
    d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;  // the counter at the decision (:278)
    d_gnss_synchro->Acq_doppler_step = d_doppler_step;
    return d_test_statistics;
}

// estimate_Doppler (:346-419) on the device
int pcps_acquisition_fine_doppler_mi355x::estimate_Doppler()
{
    gsdr_acq_fine_request rq{};
    rq.code_phase = static_cast<uint32_t>(static_cast<int>(d_gnss_synchro->Acq_delay_samples));  // shift_index (:365)
    rq.coarse_doppler_hz = static_cast<float>(d_gnss_synchro->Acq_doppler_hz);
    rq.code_slot = 0;
    const float* code = reinterpret_cast<const float*>(d_code.data());
    const int rc = d_ring ? gsdr_acq_fine_doppler_stream(d_engine, d_ring, d_ring_origin + d_window_first, code, 1, &rq, 1,
                                &d_fine)
                          : gsdr_acq_fine_doppler(d_engine, d_10_ms_buffer.data(), code, 1, &rq, 1, &d_fine);
    if (rc != GSDR_OK) throw std::runtime_error(std::string("pcps_acquisition_fine_doppler_mi355x: ") + gsdr_last_error());
    if (d_fine.accepted) d_gnss_synchro->Acq_doppler_hz = d_fine.doppler_hz;  // :407-416
    return d_fft_size;
}

// general_work (:456-607)
int pcps_acquisition_fine_doppler_mi355x::work(const std::complex<float>* in, int noutput_items)
{
    int consumed = 0;
    int samples_remaining;
    switch (d_state)
        {
        case 0:  // S0. StandBy
            if (d_active == true)
                {
                    reset_grid();
                    d_n_samples_in_buffer = 0;
                    d_state = 1;
                }
            if (!acq_parameters.blocking_on_standby)
                {
                    d_sample_counter += static_cast<uint64_t>(d_fft_size);
                    consumed = d_fft_size;
                }
            if (d_state == 1) d_window_first = d_sample_counter;
            break;
        case 1:  // S1. ComputeGrid
            if (gsdr_acq_run_dwell(d_engine, in, static_cast<uint32_t>(d_well_count), d_sample_counter, &d_coarse) != GSDR_OK)
                throw std::runtime_error(std::string("pcps_acquisition_fine_doppler_mi355x: ") + gsdr_last_error());
            if (d_dump && d_channel == d_dump_channel)
                {
                    // grid_ (:234-238): this block's |R|^2 rows added on the host
                    d_grid_tmp.resize(d_grid.size());
                    if (gsdr_acq_dump_grid(d_engine, in, 0, d_grid_tmp.data()) == GSDR_OK)
                        for (size_t i = 0; i < d_grid.size(); ++i) d_grid[i] += d_grid_tmp[i];
                }
            if (static_cast<size_t>(d_n_samples_in_buffer + d_fft_size) <= d_10_ms_buffer.size())
                std::copy(in, in + d_fft_size, &d_10_ms_buffer[d_n_samples_in_buffer]);
            d_n_samples_in_buffer += d_fft_size;
            d_well_count++;
            if (d_well_count >= d_max_dwells) d_state = 2;
            d_sample_counter += static_cast<uint64_t>(d_fft_size);
            consumed = d_fft_size;
            break;
        case 2:  // Compute test statistics and decide
            d_test_statistics = compute_CAF();
            if (d_test_statistics > d_threshold)
                d_state = 3;  // perform fine doppler estimation
            else
                {
                    d_state = 5;  // negative acquisition
                    d_n_samples_in_buffer = 0;
                }
            break;
        case 3:  // Fine doppler estimation
            samples_remaining = 10 * d_samples_per_ms - d_n_samples_in_buffer;
            if (samples_remaining > noutput_items)
                {
                    if (!d_ring) std::copy(in, in + noutput_items, &d_10_ms_buffer[d_n_samples_in_buffer]);
                    d_n_samples_in_buffer += noutput_items;
                    d_sample_counter += static_cast<uint64_t>(noutput_items);
                    consumed = noutput_items;
                }
            else
                {
                    if (samples_remaining > 0)
                        {
                            if (!d_ring) std::copy(in, in + samples_remaining, &d_10_ms_buffer[d_n_samples_in_buffer]);
                            d_sample_counter += static_cast<uint64_t>(samples_remaining);
                            consumed = samples_remaining;
                        }
                    estimate_Doppler();
                    d_n_samples_in_buffer = 0;
                    d_state = 4;
                }
            break;
        case 4:  // Positive_Acq
        case 5:  // Negative_Acq
            d_positive_acq = d_state == 4 ? 1 : 0;
            d_active = false;
            if (d_dump && d_channel == d_dump_channel) dump_results(d_fft_size);
            if (d_events) d_events(d_state == 4 ? 1 : 2);
            d_state = 0;
            if (!acq_parameters.blocking_on_standby)
                {
                    d_sample_counter += static_cast<uint64_t>(noutput_items);
                    consumed = noutput_items;
                }
            break;
        default:
            d_state = 0;
            if (!acq_parameters.blocking_on_standby)
                {
                    d_sample_counter += static_cast<uint64_t>(noutput_items);
                    consumed = noutput_items;
                }
            break;
        }
    return consumed;
}

// dump_results (:609-685): the reference's variable names, classes and dimensions
// (input_power is written as 0, :670-673); Level-5 MAT-file (mat5_writer.h)
void pcps_acquisition_fine_doppler_mi355x::dump_results(int effective_fft_size)
{
    d_dump_number++;
    std::string fn = d_dump_filename + "_";
    fn.append(1, d_gnss_synchro->System);
    fn += "_";
    fn.append(1, d_gnss_synchro->Signal[0]);
    fn.append(1, d_gnss_synchro->Signal[1]);
    fn += "_ch_" + std::to_string(d_channel) + "_" + std::to_string(d_dump_number) + "_sat_" +
          std::to_string(d_gnss_synchro->PRN) + ".mat";
    Mat5Writer m;
    if (!m.open(fn))
        {
            std::cout << "Unable to create or open Acquisition dump file\n";
            d_dump = false;
            return;
        }
    m.write("acq_grid", Mat5Writer::kSingle, static_cast<uint32_t>(effective_fft_size),
        static_cast<uint32_t>(d_num_doppler_points), d_grid.data());
    m.write_int32("doppler_max", d_config_doppler_max);
    m.write_int32("doppler_step", static_cast<int32_t>(d_doppler_step));
    m.write_int32("d_positive_acq", d_positive_acq);
    m.write_single("acq_doppler_hz", static_cast<float>(d_gnss_synchro->Acq_doppler_hz));
    m.write_single("acq_delay_samples", static_cast<float>(d_gnss_synchro->Acq_delay_samples));
    m.write_single("test_statistic", d_test_statistics);
    m.write_single("threshold", d_threshold);
    m.write_single("input_power", 0.0F);
    m.write_uint64("sample_counter", d_sample_counter);
    m.write_uint32("PRN", d_gnss_synchro->PRN);
    if (m.close()) d_last_dump = fn;
}
