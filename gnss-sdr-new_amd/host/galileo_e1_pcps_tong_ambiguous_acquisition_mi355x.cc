#include "galileo_e1_pcps_tong_ambiguous_acquisition_mi355x.h"

#include <algorithm>
#include <cmath>
#include <iostream>

#include "gnss_replicas.h"

namespace
{
constexpr double GALILEO_E1_CODE_CHIP_RATE_CPS = 1.023e6;  // Galileo_E1.h
constexpr double GALILEO_E1_B_CODE_LENGTH_CHIPS = 4092.0;
}  // namespace

// galileo_e1_pcps_tong_ambiguous_acquisition.cc:49-121
GalileoE1PcpsTongAmbiguousAcquisitionMI355X::GalileoE1PcpsTongAmbiguousAcquisitionMI355X(
    const ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams,
    unsigned int out_streams, int device)
    : PcpsTongAcquisitionAdapterMI355X(configuration, role, 4000000, 4)
{
    if (sampled_ms_ % 4 != 0)
        {
            sampled_ms_ = static_cast<unsigned int>(static_cast<int>(sampled_ms_ / 4) * 4);
            std::cerr << "coherent_integration_time should be multiple of Galileo code length (4 ms). "
                         "coherent_integration_time = "
                      << sampled_ms_ << " ms will be used.\n";
        }
    // -- Find number of samples per spreading code (4 ms)
    code_length_ = static_cast<unsigned int>(
        std::round(static_cast<double>(fs_in_) / (GALILEO_E1_CODE_CHIP_RATE_CPS / GALILEO_E1_B_CODE_LENGTH_CHIPS)));
    vector_length_ = code_length_ * static_cast<unsigned int>(static_cast<int>(sampled_ms_ / 4));
    const auto samples_per_ms = static_cast<int>(code_length_) / 4;
    make_block(samples_per_ms, in_streams, out_streams, device);
}

void GalileoE1PcpsTongAmbiguousAcquisitionMI355X::set_local_code()
{
    const bool cboc = configuration_->property("Acquisition" + std::to_string(channel_) + ".cboc", false);
    const char signal[3] = {gnss_synchro_->Signal[0], gnss_synchro_->Signal[1], '\0'};
    auto code = galileo_e1_code_gen_complex_sampled(signal, cboc, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, false);
    code.resize(code_length_);
    for (unsigned int i = 0; i < sampled_ms_ / 4; i++) std::copy_n(code.data(), code_length_, code_.data() + i * code_length_);
    acquisition_->set_local_code(code_.data());
}
