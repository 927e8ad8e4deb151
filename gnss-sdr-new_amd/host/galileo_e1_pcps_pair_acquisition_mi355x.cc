#include "galileo_e1_pcps_pair_acquisition_mi355x.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"

namespace
{
constexpr double GALILEO_E1_CODE_CHIP_RATE_CPS = 1.023e6;  // Galileo_E1.h
constexpr double GALILEO_E1_B_CODE_LENGTH_CHIPS = 4092.0;
}  // namespace

// galileo_e1_pcps_cccwsr_ambiguous_acquisition.cc:27-112,
// galileo_e1_pcps_8ms_ambiguous_acquisition.cc:35-118: the same text but for the code buffers
GalileoE1PairAcquisitionMI355X::GalileoE1PairAcquisitionMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device, Pair_Acq_Conf::Policy policy)
    : AcquisitionItemAdapterMI355X(configuration, role, 4000000, 4, "../data/acquisition.dat")
{
    if (sampled_ms_ % 4 != 0)
        {
            sampled_ms_ = static_cast<unsigned int>(static_cast<int>(sampled_ms_ / 4) * 4);
            std::cerr << "coherent_integration_time should be multiple of Galileo code length (4 ms). "
                         "coherent_integration_time = "
                      << sampled_ms_ << " ms will be used.\n";
        }
    max_dwells_ = static_cast<unsigned int>(configuration_->property(role + ".max_dwells", 1));

    // -- Find number of samples per spreading code (4 ms)
    code_length_ = static_cast<unsigned int>(
        std::round(static_cast<double>(fs_in_) / (GALILEO_E1_CODE_CHIP_RATE_CPS / GALILEO_E1_B_CODE_LENGTH_CHIPS)));
    vector_length_ = code_length_ * static_cast<unsigned int>(static_cast<int>(sampled_ms_ / 4));
    const int samples_per_ms = static_cast<int>(code_length_) / 4;

    Pair_Acq_Conf conf;
    conf.policy = policy;
    conf.sampled_ms = sampled_ms_;
    conf.max_dwells = max_dwells_;
    conf.doppler_max = doppler_max_;
    conf.fs_in = fs_in_;
    conf.samples_per_ms = samples_per_ms;
    conf.samples_per_code = static_cast<int32_t>(code_length_);
    // MI355X extension, as in the other adapters: the grid's carrier model
    const std::string carrier = configuration_->property(role + ".mi355x_carrier", std::string("exact"));
    if (carrier != "exact" && carrier != "generic" && carrier != "avx2")
        throw std::invalid_argument(role + ".mi355x_carrier must be exact, generic or avx2");
    conf.wipeoff_mode = carrier == "generic" ? GSDR_WIPE_GENERIC : (carrier == "avx2" ? GSDR_WIPE_AVX2 : GSDR_WIPE_EXACT);

    warn_item_type();
    acquisition_ = std::make_unique<pcps_pair_acquisition_mi355x>(conf, device);
    attach_block(acquisition_.get(), in_streams, out_streams);
}

// ---------------------------------------------------------------- CCCWSR
GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X::GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X(
    const ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams,
    unsigned int out_streams, int device)
    : GalileoE1PairAcquisitionMI355X(configuration, role, in_streams, out_streams, device, Pair_Acq_Conf::CCCWSR)
{
    code_data_ = std::vector<std::complex<float>>(vector_length_);
    code_pilot_ = std::vector<std::complex<float>>(vector_length_);
}

// :122-132: the configured threshold; calculate_threshold is not implemented there
void GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X::set_threshold(float threshold)
{
    threshold_ = threshold;
    acquisition_->set_threshold(threshold_);
}

// :185-205: E1-B and E1-C, one code period each at the head of a vector_length_ buffer
// (the generator fills one period; with coherent_integration_time_ms > 4 the rest stays zero)
void GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X::set_local_code()
{
    const bool cboc = configuration_->property("Acquisition" + std::to_string(channel_) + ".cboc", false);
    const auto data = galileo_e1_code_gen_complex_sampled("1B", cboc, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, false);
    const auto pilot = galileo_e1_code_gen_complex_sampled("1C", cboc, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, false);
    std::copy_n(data.begin(), std::min<size_t>(data.size(), vector_length_), code_data_.begin());
    std::copy_n(pilot.begin(), std::min<size_t>(pilot.size(), vector_length_), code_pilot_.begin());
    acquisition_->set_local_code(code_data_.data(), code_pilot_.data());
}

// ---------------------------------------------------------------- 8 ms
GalileoE1Pcps8msAmbiguousAcquisitionMI355X::GalileoE1Pcps8msAmbiguousAcquisitionMI355X(
    const ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams,
    unsigned int out_streams, int device)
    : GalileoE1PairAcquisitionMI355X(configuration, role, in_streams, out_streams, device, Pair_Acq_Conf::PCPS_8MS)
{
    code_ = std::vector<std::complex<float>>(vector_length_);
}

// :121-124
void GalileoE1Pcps8msAmbiguousAcquisitionMI355X::stop_acquisition() { acquisition_->set_active(false); }

// :203-226: the code of the synchro's signal, repeated sampled_ms / 4 times
void GalileoE1Pcps8msAmbiguousAcquisitionMI355X::set_local_code()
{
    const bool cboc = configuration_->property("Acquisition" + std::to_string(channel_) + ".cboc", false);
    const char signal[3] = {gnss_synchro_->Signal[0], gnss_synchro_->Signal[1], '\0'};
    auto code = galileo_e1_code_gen_complex_sampled(signal, cboc, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, false);
    code.resize(code_length_);
    for (unsigned int i = 0; i < sampled_ms_ / 4; i++) std::copy_n(code.data(), code_length_, code_.data() + i * code_length_);
    acquisition_->set_local_code(code_.data());
}

// :239-257: the exponential distribution's quantile with lambda = vector_length_, in double
float GalileoE1Pcps8msAmbiguousAcquisitionMI355X::calculate_threshold(float pfa) const
{
    return AcquisitionItemAdapterMI355X::calculate_threshold(pfa, vector_length_, static_cast<double>(vector_length_));
}
