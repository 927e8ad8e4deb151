#include "gps_l1_ca_pcps_acquisition_fine_doppler_mi355x.h"

#include <cmath>
#include <iostream>

#include "acq_conf.h"
#include "gnss_replicas.h"
#include "gnss_sdr_flags.h"

namespace
{
constexpr double GPS_L1_CA_CODE_RATE_CPS = 1.023e6;  // GPS_L1_CA.h
constexpr double GPS_L1_CA_CODE_LENGTH_CHIPS = 1023.0;
constexpr double GPS_L1_CA_CHIP_PERIOD_S = 9.7752e-07;
}  // namespace

// gps_l1_ca_pcps_acquisition_fine_doppler.cc:30-95
GpsL1CaPcpsAcquisitionFineDopplerMI355X::GpsL1CaPcpsAcquisitionFineDopplerMI355X(
    const ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams,
    unsigned int out_streams, int device)
    : role_(role)
{
    const std::string default_item_type("gr_complex");
    const std::string default_dump_filename = "./acquisition.mat";
    Acq_Conf acq_parameters = Acq_Conf();

    item_type_ = configuration->property(role + ".item_type", default_item_type);
    const int64_t fs_in_deprecated = configuration->property("GNSS-SDR.internal_fs_hz", static_cast<int64_t>(2048000));
    fs_in_ = configuration->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    acq_parameters.fs_in = fs_in_;
    acq_parameters.samples_per_chip =
        static_cast<unsigned int>(std::ceil(GPS_L1_CA_CHIP_PERIOD_S * static_cast<float>(acq_parameters.fs_in)));
    dump_ = configuration->property(role + ".dump", false);
    acq_parameters.dump = dump_;
    dump_filename_ = configuration->property(role + ".dump_filename", default_dump_filename);
    acq_parameters.dump_filename = dump_filename_;
    doppler_max_ = configuration->property(role + ".doppler_max", 5000);
    if (FLAGS_doppler_max != 0) doppler_max_ = FLAGS_doppler_max;
    acq_parameters.doppler_max = doppler_max_;
    sampled_ms_ = configuration->property(role + ".coherent_integration_time_ms", 1U);
    acq_parameters.sampled_ms = sampled_ms_;
    max_dwells_ = configuration->property(role + ".max_dwells", 1U);
    acq_parameters.max_dwells = max_dwells_;
    acq_parameters.blocking_on_standby = configuration->property(role + ".blocking_on_standby", false);
    // MI355X extension, as in the other adapters: the coarse grid's carrier model
    acq_parameters.mi355x_carrier = configuration->property(role + ".mi355x_carrier", std::string("exact"));

    // -- Find number of samples per spreading code
    vector_length_ = static_cast<unsigned int>(
        std::round(static_cast<double>(fs_in_) / (GPS_L1_CA_CODE_RATE_CPS / GPS_L1_CA_CODE_LENGTH_CHIPS)));
    acq_parameters.samples_per_ms = static_cast<float>(vector_length_);
    code_ = std::vector<std::complex<float>>(vector_length_);

    // the reference builds the gr_complex block whatever the item type says, with a warning
    item_size_ = sizeof(std::complex<float>);
    if (item_type_ != "gr_complex") std::cerr << item_type_ << " unknown acquisition item type\n";
    acquisition_ = std::make_unique<pcps_acquisition_fine_doppler_mi355x>(acq_parameters, device);

    if (in_streams > 1) std::cerr << "This implementation only supports one input stream\n";
    if (out_streams > 0) std::cerr << "This implementation does not provide an output stream\n";
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::stop_acquisition()
{
    acquisition_->set_state(0);
    acquisition_->set_active(false);
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_threshold(float threshold)
{
    threshold_ = threshold;
    acquisition_->set_threshold(threshold_);
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_doppler_max(unsigned int doppler_max)
{
    doppler_max_ = static_cast<int>(doppler_max);
    acquisition_->set_doppler_max(doppler_max_);
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_doppler_step(unsigned int doppler_step)
{
    doppler_step_ = doppler_step;
    acquisition_->set_doppler_step(doppler_step_);
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_gnss_synchro(Gnss_Synchro* gnss_synchro)
{
    gnss_synchro_ = gnss_synchro;
    acquisition_->set_gnss_synchro(gnss_synchro_);
}

void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_channel(unsigned int channel)
{
    channel_ = channel;
    acquisition_->set_channel(channel_);
}

// :145-149
void GpsL1CaPcpsAcquisitionFineDopplerMI355X::set_local_code()
{
    code_ = gps_l1_ca_code_gen_complex_sampled(gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0);
    code_.resize(vector_length_);
    acquisition_->set_local_code(code_.data());
}
