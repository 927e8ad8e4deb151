#include "gps_l1_ca_pcps_quicksync_acquisition_mi355x.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"

namespace
{
constexpr double GPS_L1_CA_CODE_RATE_CPS = 1.023e6;  // GPS_L1_CA.h
constexpr double GPS_L1_CA_CODE_LENGTH_CHIPS = 1023.0;
}  // namespace

// gps_l1_ca_pcps_quicksync_acquisition.cc:36-145
GpsL1CaPcpsQuickSyncAcquisitionMI355X::GpsL1CaPcpsQuickSyncAcquisitionMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : AcquisitionItemAdapterMI355X(configuration, role, 2048000, 4, "./data/acquisition.dat")
{
    // -- Find number of samples per spreading code
    code_length_ = static_cast<unsigned int>(
        std::round(static_cast<double>(fs_in_) / (GPS_L1_CA_CODE_RATE_CPS / GPS_L1_CA_CODE_LENGTH_CHIPS)));

    // the folding factor of :70, unless configured
    const auto temp = static_cast<unsigned int>(std::ceil(std::sqrt(std::log2(code_length_))));
    folding_factor_ = static_cast<unsigned int>(configuration_->property(role + ".folding_factor", static_cast<int>(temp)));
    if (folding_factor_ == 0) throw std::invalid_argument(role + ".folding_factor must be positive");

    if (sampled_ms_ % folding_factor_ != 0)
        {
            std::cerr << "QuickSync Algorithm requires a coherent_integration_time multiple of " << folding_factor_
                      << "ms, Value entered " << sampled_ms_ << " ms\n";
            if (sampled_ms_ < folding_factor_)
                sampled_ms_ = folding_factor_;
            else
                sampled_ms_ = static_cast<unsigned int>(static_cast<int>(sampled_ms_ / folding_factor_)) * folding_factor_;
            std::cerr << " Coherent_integration_time of " << sampled_ms_ << " ms will be used instead.\n";
        }

    vector_length_ = code_length_ * sampled_ms_;
    bit_transition_flag_ = configuration_->property(role + ".bit_transition_flag", false);
    max_dwells_ = bit_transition_flag_ ? 2U : static_cast<unsigned int>(configuration_->property(role + ".max_dwells", 1));

    // the block is made for items of sampled_ms code periods, its stream_to_vector delivers
    // folding_factor of them (:120-126): GNU Radio connects the two only when they agree
    if (sampled_ms_ != folding_factor_)
        throw std::invalid_argument(role + ": coherent_integration_time_ms (" + std::to_string(sampled_ms_) +
                                    " after rounding) must equal folding_factor (" + std::to_string(folding_factor_) +
                                    "): the reference's flow graph does not connect otherwise");

    const int samples_per_ms = static_cast<int>(std::round(code_length_));
    code_ = std::vector<std::complex<float>>(code_length_);

    QuickSync_Acq_Conf conf;
    conf.folding_factor = folding_factor_;
    conf.sampled_ms = sampled_ms_;
    conf.max_dwells = max_dwells_;
    conf.doppler_max = doppler_max_;
    conf.fs_in = fs_in_;
    conf.samples_per_ms = samples_per_ms;
    conf.samples_per_code = static_cast<int32_t>(code_length_);
    conf.bit_transition_flag = bit_transition_flag_;

    warn_item_type();
    acquisition_ = std::make_unique<pcps_quicksync_acquisition_mi355x>(conf, device);
    attach_block(acquisition_.get(), in_streams, out_streams);
}

// :227-243: one code period (sampled_ms / folding_factor = 1 copy)
void GpsL1CaPcpsQuickSyncAcquisitionMI355X::set_local_code()
{
    auto code = gps_l1_ca_code_gen_complex_sampled(gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0);
    code.resize(code_length_);
    std::copy_n(code.data(), code_length_, code_.data());
    acquisition_->set_local_code(code_.data());
}

// :264-281: the exponential distribution's quantile with lambda = code_length / folding_factor
float GpsL1CaPcpsQuickSyncAcquisitionMI355X::calculate_threshold(float pfa) const
{
    return AcquisitionItemAdapterMI355X::calculate_threshold(pfa, code_length_ / folding_factor_,
        static_cast<double>(code_length_) / static_cast<double>(folding_factor_));
}
