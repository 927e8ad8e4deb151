#include "gps_l1_ca_pcps_tong_acquisition_mi355x.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "gnss_replicas.h"

namespace
{
constexpr double GPS_L1_CA_CODE_RATE_CPS = 1.023e6;  // GPS_L1_CA.h
constexpr double GPS_L1_CA_CODE_LENGTH_CHIPS = 1023.0;
}  // namespace

// gps_l1_ca_pcps_tong_acquisition.cc:49-72 and galileo_e1_pcps_tong_ambiguous_acquisition.cc:49-82
PcpsTongAcquisitionAdapterMI355X::PcpsTongAcquisitionAdapterMI355X(const ConfigurationInterface* configuration,
    const std::string& role, int64_t default_fs, int default_ms)
    : AcquisitionItemAdapterMI355X(configuration, role, default_fs, default_ms, "./data/acquisition.dat")
{
    tong_init_val_ = static_cast<unsigned int>(configuration_->property(role + ".tong_init_val", 1));
    tong_max_val_ = static_cast<unsigned int>(configuration_->property(role + ".tong_max_val", 2));
    tong_max_dwells_ = static_cast<unsigned int>(
        configuration_->property(role + ".tong_max_dwells", static_cast<int>(tong_max_val_) + 1));
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

    warn_item_type();
    acquisition_ = std::make_unique<pcps_tong_acquisition_mi355x>(conf, device);
    // the block reads sampled_ms * samples_per_ms samples of the vectors it is fed
    if (acquisition_->fft_size() != vector_length_)
        throw std::invalid_argument(role_ + ": items of " + std::to_string(vector_length_) + " samples for a block of " +
                                    std::to_string(acquisition_->fft_size()) +
                                    ": the reference's flow graph does not connect");
    attach_block(acquisition_.get(), in_streams, out_streams);
}

float PcpsTongAcquisitionAdapterMI355X::calculate_threshold(float pfa) const
{
    return AcquisitionItemAdapterMI355X::calculate_threshold(pfa, vector_length_, static_cast<double>(vector_length_));
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
