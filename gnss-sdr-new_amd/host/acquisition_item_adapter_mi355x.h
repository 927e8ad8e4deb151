// Shared body of the adapters of the item-wise acquisition blocks on the MI355X engine
// (acquisition_item_block_mi355x.h): Tong, QuickSync, the two Galileo E1 paired-code ones and the
// E5a IQ-CAF one.  As pcps_acquisition_adapter.h does for the plain PCPS adapters, it holds what
// the reference repeats in every one of them: the common keys (item_type,
// GNSS-SDR.internal_fs_sps over internal_fs_hz, dump, doppler_max with FLAGS_doppler_max over it,
// coherent_integration_time_ms, dump_filename), the warnings, the setters forwarded to the block,
// reset = set_active(true), the pfa-or-configured threshold and the exponential quantile behind
// it.  An adapter supplies its defaults, its own keys, its lengths, its block and its replica
// (set_local_code).  A new item-wise mode's adapter starts as a class derived from this one.
#ifndef GSDR_HOST_ACQUISITION_ITEM_ADAPTER_MI355X_H
#define GSDR_HOST_ACQUISITION_ITEM_ADAPTER_MI355X_H

#include <complex>
#include <memory>
#include <string>

#include "acquisition_interface.h"
#include "acquisition_item_block_mi355x.h"
#include "configuration.h"

class AcquisitionItemAdapterMI355X : public AcquisitionInterface
{
public:
    std::string role() override { return role_; }
    size_t item_size() override { return item_size_; }

    void set_gnss_synchro(Gnss_Synchro* gnss_synchro) override;
    void set_channel(unsigned int channel) override;
    // the block publishes its events itself; the reference's adapters keep no FSM either
    void set_channel_fsm(std::weak_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = std::move(channel_fsm); }
    // per-channel pfa, then the role's; without one, the configured threshold
    void set_threshold(float threshold) override;
    void set_doppler_max(unsigned int doppler_max) override;
    void set_doppler_step(unsigned int doppler_step) override;
    void init() override { block_->init(); }
    void set_state(int state) override { block_->set_state(state); }
    signed int mag() override { return static_cast<signed int>(block_->mag()); }
    void reset() override { block_->set_active(true); }
    void stop_acquisition() override;
    void set_resampler_latency(uint32_t latency_samples __attribute__((unused))) override {}
    // the adapter's threshold for a probability of false alarm
    virtual float calculate_threshold(float pfa) const = 0;

    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int doppler_max() const { return doppler_max_; }
    float threshold() const { return threshold_; }

protected:
    // the keys the adapters read alike; default_fs is GNSS-SDR.internal_fs_hz's default, default_ms
    // coherent_integration_time_ms's
    AcquisitionItemAdapterMI355X(const ConfigurationInterface* configuration, const std::string& role, int64_t default_fs,
        int default_ms, const std::string& default_dump_filename);
    // the reference builds the gr_complex block only; any other item type gets a warning
    void warn_item_type() const;
    // the block the calls above go to (the adapter owns it), and the stream-count warnings
    void attach_block(acquisition_item_block_mi355x* block, unsigned int in_streams, unsigned int out_streams);
    // quantile(exponential_distribution(lambda), (1 - pfa)^(1 / cells)) over cells_per_row cells in
    // each Doppler row of the grid
    float calculate_threshold(float pfa, unsigned int cells_per_row, double lambda) const;

    const ConfigurationInterface* configuration_;
    acquisition_item_block_mi355x* block_{nullptr};
    std::weak_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_{nullptr};
    std::string item_type_;
    std::string dump_filename_;
    std::string role_;
    int64_t fs_in_;
    size_t item_size_{sizeof(std::complex<float>)};
    float threshold_{0.0F};
    unsigned int doppler_max_;
    unsigned int vector_length_{0};
    unsigned int code_length_{0};
    unsigned int channel_{0};
    unsigned int doppler_step_{0};
    unsigned int sampled_ms_;
    bool dump_;
};

#endif
