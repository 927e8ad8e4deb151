// GPS L1 C/A fine-Doppler PCPS acquisition adapter on the MI355X engine: the counterpart
// of GpsL1CaPcpsAcquisitionFineDoppler (src/algorithms/acquisition/adapters/
// gps_l1_ca_pcps_acquisition_fine_doppler.{h,cc}), selected in a .conf with
//   Acquisition_1C.implementation=GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_MI355X
// Same keys and defaults (:38-68): item_type, GNSS-SDR.internal_fs_sps (2048000), dump,
// dump_filename (./acquisition.mat), doppler_max (5000), coherent_integration_time_ms (1),
// max_dwells (1), blocking_on_standby (false).
#ifndef GSDR_HOST_GPS_L1_CA_PCPS_ACQUISITION_FINE_DOPPLER_MI355X_H
#define GSDR_HOST_GPS_L1_CA_PCPS_ACQUISITION_FINE_DOPPLER_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_interface.h"
#include "configuration.h"
#include "pcps_acquisition_fine_doppler_mi355x.h"

class GpsL1CaPcpsAcquisitionFineDopplerMI355X : public AcquisitionInterface
{
public:
    GpsL1CaPcpsAcquisitionFineDopplerMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);

    std::string role() override { return role_; }
    std::string implementation() override { return "GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_MI355X"; }
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

    // the gr::block the reference connects into the flowgraph (get_left_block)
    pcps_acquisition_fine_doppler_mi355x* get_block() { return acquisition_.get(); }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int max_dwells() const { return max_dwells_; }
    int doppler_max() const { return doppler_max_; }

private:
    std::unique_ptr<pcps_acquisition_fine_doppler_mi355x> acquisition_;
    std::vector<std::complex<float>> code_;
    std::weak_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_{nullptr};
    std::string item_type_;
    std::string dump_filename_;
    std::string role_;
    int64_t fs_in_;
    size_t item_size_;
    float threshold_{0.0F};
    int doppler_max_;
    unsigned int vector_length_;
    unsigned int channel_{0};
    unsigned int doppler_step_{0};
    unsigned int sampled_ms_;
    unsigned int max_dwells_;
    bool dump_;
};

#endif
