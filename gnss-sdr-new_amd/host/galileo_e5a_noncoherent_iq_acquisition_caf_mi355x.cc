#include "galileo_e5a_noncoherent_iq_acquisition_caf_mi355x.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"

namespace
{
constexpr double GALILEO_E5A_CODE_CHIP_RATE_CPS = 1.023e7;  // Galileo_E5a.h
constexpr double GALILEO_E5A_CODE_LENGTH_CHIPS = 10230.0;
}  // namespace

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::load_code_table(const ConfigurationInterface* configuration,
    const std::string& role)
{
    const char* env = std::getenv("GSDR_GALILEO_E5A_CODES");
    const std::string path = configuration->property(role + ".e5a_code_table", std::string(env ? env : ""));
    std::string why;
    if (path.empty())
        throw std::invalid_argument(role + ": the Galileo E5a primary codes are not shipped: name a code table with " + role +
                                    ".e5a_code_table or GSDR_GALILEO_E5A_CODES (layout: gnss_replicas.h)");
    if (!galileo_e5a_load_code_table(path, &why)) throw std::invalid_argument(role + ": " + why);
}

// galileo_e5a_noncoherent_iq_acquisition_caf.cc:41-127
GalileoE5aNoncoherentIQAcquisitionCafMI355X::GalileoE5aNoncoherentIQAcquisitionCafMI355X(
    const ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams,
    unsigned int out_streams, int device)
    : AcquisitionItemAdapterMI355X(configuration, role, 32000000, 1, "../data/acquisition.dat")
{
    CAF_window_hz_ = configuration_->property(role + ".CAF_window_hz", 0);
    Zero_padding = configuration_->property(role + ".Zero_padding", 0);
    if (sampled_ms_ > 3)
        {
            sampled_ms_ = 3;
            std::cout << "Too high coherent integration time. Changing to 3ms\n";
        }
    if (Zero_padding > 0)
        {
            sampled_ms_ = 2;
            std::cout << "Zero padding activated. Changing to 1ms code + 1ms zero padding\n";
        }
    max_dwells_ = static_cast<unsigned int>(configuration_->property(role + ".max_dwells", 1));
    bit_transition_flag_ = configuration_->property(role + ".bit_transition_flag", false);

    // samples per spreading code (1 ms)
    code_length_ = static_cast<unsigned int>(std::round(
        static_cast<double>(fs_in_) / GALILEO_E5A_CODE_CHIP_RATE_CPS * GALILEO_E5A_CODE_LENGTH_CHIPS));
    vector_length_ = code_length_ * sampled_ms_;
    codeI_ = std::vector<std::complex<float>>(vector_length_);
    codeQ_ = std::vector<std::complex<float>>(vector_length_);

    const bool enable_monitor_output = configuration_->property("AcquisitionMonitor.enable_monitor", false);
    const std::string sig = configuration_->property("Channel.signal", std::string("5X"));
    if (sig.size() >= 2 && sig[0] == '5' && sig[1] == 'X') both_signal_components = true;

    E5a_Iq_Caf_Acq_Conf conf;
    conf.sampled_ms = sampled_ms_;
    conf.max_dwells = max_dwells_;
    conf.doppler_max = doppler_max_;
    conf.fs_in = fs_in_;
    conf.samples_per_ms = static_cast<int32_t>(code_length_);
    conf.samples_per_code = static_cast<int32_t>(code_length_);
    conf.bit_transition_flag = bit_transition_flag_;
    conf.both_signal_components = both_signal_components;
    conf.CAF_window_hz = CAF_window_hz_;
    conf.Zero_padding = Zero_padding;
    conf.enable_monitor_output = enable_monitor_output;

    warn_item_type();
    acquisition_ = std::make_unique<galileo_e5a_noncoherentIQ_acquisition_caf_mi355x>(conf, device);
    attach_block(acquisition_.get(), in_streams, out_streams);
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_local_code()
{
    std::vector<std::complex<float>> codeI(code_length_), codeQ(code_length_);
    const bool x = gnss_synchro_->Signal[0] == '5' && gnss_synchro_->Signal[1] == 'X';
    const auto fs = static_cast<int32_t>(fs_in_);
    bool ok;
    if (x)
        ok = galileo_e5_a_code_gen_complex_sampled(codeI, gnss_synchro_->PRN, "5I", fs, 0) &&
             galileo_e5_a_code_gen_complex_sampled(codeQ, gnss_synchro_->PRN, "5Q", fs, 0);
    else
        // as the reference has it (:229-234): any other signal gets the 5X row, I + jQ
        ok = galileo_e5_a_code_gen_complex_sampled(codeI, gnss_synchro_->PRN, "5X", fs, 0);
    if (!ok) throw std::invalid_argument(role_ + ": no Galileo E5a code for PRN " + std::to_string(gnss_synchro_->PRN));
    // the secondary sequence (1, 1, 1) here; the block makes the other one
    std::fill(codeI_.begin(), codeI_.end(), std::complex<float>(0.0F, 0.0F));
    std::fill(codeQ_.begin(), codeQ_.end(), std::complex<float>(0.0F, 0.0F));
    const unsigned int periods = Zero_padding == 0 ? sampled_ms_ : 1U;  // else 1 ms of code + 1 ms of zeros
    for (unsigned int i = 0; i < periods; i++)
        {
            std::copy_n(codeI.data(), code_length_, codeI_.data() + i * code_length_);
            if (x) std::copy_n(codeQ.data(), code_length_, codeQ_.data() + i * code_length_);
        }
    acquisition_->set_local_code(codeI_.data(), codeQ_.data());
}

float GalileoE5aNoncoherentIQAcquisitionCafMI355X::calculate_threshold(float pfa) const
{
    return AcquisitionItemAdapterMI355X::calculate_threshold(pfa, vector_length_, static_cast<double>(vector_length_));
}
