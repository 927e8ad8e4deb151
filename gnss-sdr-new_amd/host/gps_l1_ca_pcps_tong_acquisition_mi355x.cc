#include "gps_l1_ca_pcps_tong_acquisition_mi355x.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"
#include "gnss_sdr_flags.h"

namespace
{
constexpr double GPS_L1_CA_CODE_RATE_CPS = 1.023e6;  // GPS_L1_CA.h
constexpr double GPS_L1_CA_CODE_LENGTH_CHIPS = 1023.0;
}  // namespace

// gps_l1_ca_pcps_tong_acquisition.cc:49-72 and galileo_e1_pcps_tong_ambiguous_acquisition.cc:49-82
PcpsTongAcquisitionAdapterMI355X::PcpsTongAcquisitionAdapterMI355X(const ConfigurationInterface* configuration,
    const std::string& role, int64_t default_fs, int default_ms)
    : configuration_(configuration), role_(role)
{
    const std::string default_item_type("gr_complex");
    const std::string default_dump_filename("./data/acquisition.dat");

    item_type_ = configuration_->property(role + ".item_type", default_item_type);
    const int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", default_fs);
    fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    dump_ = configuration_->property(role + ".dump", false);
    doppler_max_ = static_cast<unsigned int>(configuration_->property(role + ".doppler_max", 5000));
    if (FLAGS_doppler_max != 0) doppler_max_ = static_cast<unsigned int>(FLAGS_doppler_max);
    sampled_ms_ = static_cast<unsigned int>(configuration_->property(role + ".coherent_integration_time_ms", default_ms));

    tong_init_val_ = static_cast<unsigned int>(configuration_->property(role + ".tong_init_val", 1));
    tong_max_val_ = static_cast<unsigned int>(configuration_->property(role + ".tong_max_val", 2));
    tong_max_dwells_ = static_cast<unsigned int>(
        configuration_->property(role + ".tong_max_dwells", static_cast<int>(tong_max_val_) + 1));

    dump_filename_ = configuration_->property(role + ".dump_filename", default_dump_filename);
    enable_monitor_output_ = configuration_->property("AcquisitionMonitor.enable_monitor", false);
}

void PcpsTongAcquisitionAdapterMI355X::make_block(int samples_per_ms, unsigned int in_streams, unsigned int out_streams,
    int device)
{
    code_ = std::vector<std::complex<float>>(vector_length_);

    Tong_Acq_Conf conf;
    conf.sampled_ms = sampled_ms_;
    conf.doppler_max = doppler_max_;
    conf.fs_in = fs_in_;
    conf.samples_per_ms = samples_per_ms;
    conf.samples_per_code = static_cast<int32_t>(code_length_);
    conf.tong_init_val = tong_init_val_;
    conf.tong_max_val = tong_max_val_;
    conf.tong_max_dwells = tong_max_dwells_;
    conf.enable_monitor_output = enable_monitor_output_;

    // the reference builds the gr_complex block only; any other item type gets a warning
    if (item_type_ != "gr_complex") std::cerr << item_type_ << " unknown acquisition item type\n";
    acquisition_ = std::make_unique<pcps_tong_acquisition_mi355x>(conf, device);
    // the block reads sampled_ms * samples_per_ms samples of the vectors it is fed
    if (acquisition_->fft_size() != vector_length_)
        throw std::invalid_argument(role_ + ": items of " + std::to_string(vector_length_) + " samples for a block of " +
                                    std::to_string(acquisition_->fft_size()) +
                                    ": the reference's flow graph does not connect");

    if (in_streams > 1) std::cerr << "This implementation only supports one input stream\n";
    if (out_streams > 0) std::cerr << "This implementation does not provide an output stream\n";
}

void PcpsTongAcquisitionAdapterMI355X::stop_acquisition()
{
    acquisition_->set_state(0);
    acquisition_->set_active(false);
}

// per-channel pfa, then the role's; without one, the configured threshold
void PcpsTongAcquisitionAdapterMI355X::set_threshold(float threshold)
{
    float pfa = configuration_->property(role_ + std::to_string(channel_) + ".pfa", 0.0F);
    if (pfa == 0.0) pfa = configuration_->property(role_ + ".pfa", 0.0F);
    threshold_ = pfa == 0.0 ? threshold : calculate_threshold(pfa);
    acquisition_->set_threshold(threshold_);
}

void PcpsTongAcquisitionAdapterMI355X::set_doppler_max(unsigned int doppler_max)
{
    doppler_max_ = doppler_max;
    acquisition_->set_doppler_max(doppler_max_);
}

void PcpsTongAcquisitionAdapterMI355X::set_doppler_step(unsigned int doppler_step)
{
    doppler_step_ = doppler_step;
    acquisition_->set_doppler_step(doppler_step_);
}

void PcpsTongAcquisitionAdapterMI355X::set_gnss_synchro(Gnss_Synchro* gnss_synchro)
{
    gnss_synchro_ = gnss_synchro;
    acquisition_->set_gnss_synchro(gnss_synchro_);
}

void PcpsTongAcquisitionAdapterMI355X::set_channel(unsigned int channel)
{
    channel_ = channel;
    acquisition_->set_channel(channel_);
}

float PcpsTongAcquisitionAdapterMI355X::calculate_threshold(float pfa) const
{
    // (the reference's loop does not end with a zero step)
    if (doppler_step_ == 0) throw std::invalid_argument(role_ + ": set_doppler_step before a pfa threshold");
    unsigned int frequency_bins = 0;
    for (int doppler = -static_cast<int>(doppler_max_); doppler <= static_cast<int>(doppler_max_);
         doppler += static_cast<int>(doppler_step_))
        frequency_bins++;
    const unsigned int ncells = vector_length_ * frequency_bins;
    const double exponent = 1 / static_cast<double>(ncells);
    const double val = std::pow(1.0 - pfa, exponent);
    const auto lambda = static_cast<double>(vector_length_);
    // quantile(exponential_distribution(lambda), val) = -log1p(-val) / lambda
    return static_cast<float>(-std::log1p(-val) / lambda);
}

// gps_l1_ca_pcps_tong_acquisition.cc:74-106
GpsL1CaPcpsTongAcquisitionMI355X::GpsL1CaPcpsTongAcquisitionMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : PcpsTongAcquisitionAdapterMI355X(configuration, role, 2048000, 1)
{
    code_length_ = static_cast<unsigned int>(
        std::round(static_cast<double>(fs_in_) / (GPS_L1_CA_CODE_RATE_CPS / GPS_L1_CA_CODE_LENGTH_CHIPS)));
    vector_length_ = code_length_ * sampled_ms_;
    // samples_per_ms and samples_per_code are both the code length (:84-85)
    make_block(static_cast<int>(code_length_), in_streams, out_streams, device);
}

void GpsL1CaPcpsTongAcquisitionMI355X::set_local_code()
{
    auto code = gps_l1_ca_code_gen_complex_sampled(gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0);
    code.resize(code_length_);
    for (unsigned int i = 0; i < sampled_ms_; i++) std::copy_n(code.data(), code_length_, code_.data() + i * code_length_);
    acquisition_->set_local_code(code_.data());
}
