#include "galileo_e5a_noncoherent_iq_acquisition_caf_mi355x.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"
#include "gnss_sdr_flags.h"

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
    : configuration_(configuration), role_(role)
{
    const std::string default_item_type("gr_complex");
    const std::string default_dump_filename("../data/acquisition.dat");

    item_type_ = configuration_->property(role + ".item_type", default_item_type);
    const int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", static_cast<int64_t>(32000000));
    fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    dump_ = configuration_->property(role + ".dump", false);
    doppler_max_ = static_cast<unsigned int>(configuration_->property(role + ".doppler_max", 5000));
    if (FLAGS_doppler_max != 0) doppler_max_ = static_cast<unsigned int>(FLAGS_doppler_max);
    CAF_window_hz_ = configuration_->property(role + ".CAF_window_hz", 0);
    Zero_padding = configuration_->property(role + ".Zero_padding", 0);
    sampled_ms_ = static_cast<unsigned int>(configuration_->property(role + ".coherent_integration_time_ms", 1));
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
    dump_filename_ = configuration_->property(role + ".dump_filename", default_dump_filename);
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
    // the reference builds the gr_complex block only; any other item type gets a warning
    if (item_type_ != "gr_complex") std::cerr << item_type_ << " unknown acquisition item type\n";
    acquisition_ = std::make_unique<galileo_e5a_noncoherentIQ_acquisition_caf_mi355x>(conf, device);

    if (in_streams > 1) std::cerr << "This implementation only supports one input stream\n";
    if (out_streams > 0) std::cerr << "This implementation does not provide an output stream\n";
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::stop_acquisition()
{
    acquisition_->set_state(0);
    acquisition_->set_active(false);
}

// per-channel pfa, then the role's; without one, the configured threshold (:137-161)
void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_threshold(float threshold)
{
    float pfa = configuration_->property(role_ + std::to_string(channel_) + ".pfa", 0.0F);
    if (pfa == 0.0) pfa = configuration_->property(role_ + ".pfa", 0.0F);
    threshold_ = pfa == 0.0 ? threshold : calculate_threshold(pfa);
    acquisition_->set_threshold(threshold_);
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_doppler_max(unsigned int doppler_max)
{
    doppler_max_ = doppler_max;
    acquisition_->set_doppler_max(doppler_max_);
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_doppler_step(unsigned int doppler_step)
{
    doppler_step_ = doppler_step;
    acquisition_->set_doppler_step(doppler_step_);
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_gnss_synchro(Gnss_Synchro* gnss_synchro)
{
    gnss_synchro_ = gnss_synchro;
    acquisition_->set_gnss_synchro(gnss_synchro_);
}

void GalileoE5aNoncoherentIQAcquisitionCafMI355X::set_channel(unsigned int channel)
{
    channel_ = channel;
    acquisition_->set_channel(channel_);
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
