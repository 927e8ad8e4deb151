// The GPS L1 C/A QuickSync acquisition adapter on the MI355X engine: the counterpart of
// GpsL1CaPcpsQuickSyncAcquisition (src/algorithms/acquisition/adapters/
// gps_l1_ca_pcps_quicksync_acquisition.{h,cc}), selected in a .conf with
//   Acquisition_1C.implementation=GPS_L1_CA_PCPS_QuickSync_Acquisition_MI355X
// Same keys and defaults: item_type, GNSS-SDR.internal_fs_sps (2048000), doppler_max (5000,
// FLAGS_doppler_max over it), coherent_integration_time_ms (4), folding_factor
// (ceil(sqrt(log2(samples per code)))), bit_transition_flag (false; true forces max_dwells 2),
// max_dwells (1), <role><channel>.pfa and <role>.pfa.  coherent_integration_time_ms is rounded to
// a multiple of the folding factor as the reference rounds it (:73-89).  The reference builds its
// block for items of coherent_integration_time_ms code periods and feeds it vectors of
// folding_factor code periods (:120-126), a flow graph that connects only when the two agree: any
// other configuration is refused here with a message.  dump is read and not mirrored.
#ifndef GSDR_HOST_GPS_L1_CA_PCPS_QUICKSYNC_ACQUISITION_MI355X_H
#define GSDR_HOST_GPS_L1_CA_PCPS_QUICKSYNC_ACQUISITION_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_interface.h"
#include "configuration.h"
#include "pcps_quicksync_acquisition_mi355x.h"

class GpsL1CaPcpsQuickSyncAcquisitionMI355X : public AcquisitionInterface
{
public:
    GpsL1CaPcpsQuickSyncAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);

    std::string role() override { return role_; }
    std::string implementation() override { return "GPS_L1_CA_PCPS_QuickSync_Acquisition_MI355X"; }
    size_t item_size() override { return item_size_; }

    void set_gnss_synchro(Gnss_Synchro* gnss_synchro) override;
    void set_channel(unsigned int channel) override;
    // the block publishes its events itself; the reference's adapter keeps no FSM either
    void set_channel_fsm(std::weak_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = std::move(channel_fsm); }
    void set_threshold(float threshold) override;
    void set_doppler_max(unsigned int doppler_max) override;
    void set_doppler_step(unsigned int doppler_step) override;
    void init() override { acquisition_->init(); }
    void set_local_code() override;
    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return static_cast<signed int>(acquisition_->mag()); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override;
    void set_resampler_latency(uint32_t latency_samples __attribute__((unused))) override {}
    float calculate_threshold(float pfa) const;

    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_quicksync_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int folding_factor() const { return folding_factor_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    unsigned int doppler_max() const { return doppler_max_; }
    bool bit_transition_flag() const { return bit_transition_flag_; }
    float threshold() const { return threshold_; }

private:
    const ConfigurationInterface* configuration_;
    std::unique_ptr<pcps_quicksync_acquisition_mi355x> acquisition_;
    std::weak_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_{nullptr};
    std::vector<std::complex<float>> code_;
    std::string item_type_;
    std::string dump_filename_;
    std::string role_;
    int64_t fs_in_;
    size_t item_size_;
    float threshold_{0.0F};
    unsigned int doppler_max_;
    unsigned int vector_length_;
    unsigned int code_length_;
    unsigned int folding_factor_;
    unsigned int channel_{0};
    unsigned int doppler_step_{0};
    unsigned int sampled_ms_;
    unsigned int max_dwells_;
    bool bit_transition_flag_;
    bool dump_;
};

#endif
