#include "acquisition_item_adapter_mi355x.h"

#include <cmath>
#include <iostream>
#include <stdexcept>

#include "gnss_sdr_flags.h"

AcquisitionItemAdapterMI355X::AcquisitionItemAdapterMI355X(const ConfigurationInterface* configuration,
    const std::string& role, int64_t default_fs, int default_ms, const std::string& default_dump_filename)
    : configuration_(configuration), role_(role)
{
    const std::string default_item_type("gr_complex");

    item_type_ = configuration_->property(role + ".item_type", default_item_type);
    const int64_t fs_in_deprecated = configuration_->property("GNSS-SDR.internal_fs_hz", default_fs);
    fs_in_ = configuration_->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    dump_ = configuration_->property(role + ".dump", false);
    doppler_max_ = static_cast<unsigned int>(configuration_->property(role + ".doppler_max", 5000));
    if (FLAGS_doppler_max != 0) doppler_max_ = static_cast<unsigned int>(FLAGS_doppler_max);
    sampled_ms_ = static_cast<unsigned int>(configuration_->property(role + ".coherent_integration_time_ms", default_ms));
    dump_filename_ = configuration_->property(role + ".dump_filename", default_dump_filename);
}

void AcquisitionItemAdapterMI355X::warn_item_type() const
{
    if (item_type_ != "gr_complex") std::cerr << item_type_ << " unknown acquisition item type\n";
}

void AcquisitionItemAdapterMI355X::attach_block(acquisition_item_block_mi355x* block, unsigned int in_streams,
    unsigned int out_streams)
{
    block_ = block;
    if (in_streams > 1) std::cerr << "This implementation only supports one input stream\n";
    if (out_streams > 0) std::cerr << "This implementation does not provide an output stream\n";
}

void AcquisitionItemAdapterMI355X::stop_acquisition()
{
    block_->set_state(0);
    block_->set_active(false);
}

void AcquisitionItemAdapterMI355X::set_threshold(float threshold)
{
    float pfa = configuration_->property(role_ + std::to_string(channel_) + ".pfa", 0.0F);
    if (pfa == 0.0) pfa = configuration_->property(role_ + ".pfa", 0.0F);
    threshold_ = pfa == 0.0 ? threshold : calculate_threshold(pfa);
    block_->set_threshold(threshold_);
}

void AcquisitionItemAdapterMI355X::set_doppler_max(unsigned int doppler_max)
{
    doppler_max_ = doppler_max;
    block_->set_doppler_max(doppler_max_);
}

void AcquisitionItemAdapterMI355X::set_doppler_step(unsigned int doppler_step)
{
    doppler_step_ = doppler_step;
    block_->set_doppler_step(doppler_step_);
}

void AcquisitionItemAdapterMI355X::set_gnss_synchro(Gnss_Synchro* gnss_synchro)
{
    gnss_synchro_ = gnss_synchro;
    block_->set_gnss_synchro(gnss_synchro_);
}

void AcquisitionItemAdapterMI355X::set_channel(unsigned int channel)
{
    channel_ = channel;
    block_->set_channel(channel_);
}

float AcquisitionItemAdapterMI355X::calculate_threshold(float pfa, unsigned int cells_per_row, double lambda) const
{
    // (the reference's loop does not end with a zero step)
    if (doppler_step_ == 0) throw std::invalid_argument(role_ + ": set_doppler_step before a pfa threshold");
    const unsigned int ncells = cells_per_row * acquisition_doppler_bins(doppler_max_, doppler_step_);
    const double exponent = 1 / static_cast<double>(ncells);
    const double val = std::pow(1.0 - pfa, exponent);
    // quantile(exponential_distribution(lambda), val) = -log1p(-val) / lambda
    return static_cast<float>(-std::log1p(-val) / lambda);
}
