// The GPS L1 C/A Tong acquisition adapter on the MI355X engine: the counterpart of
// GpsL1CaPcpsTongAcquisition (src/algorithms/acquisition/adapters/
// gps_l1_ca_pcps_tong_acquisition.{h,cc}), selected in a .conf with
//   Acquisition_1C.implementation=GPS_L1_CA_PCPS_Tong_Acquisition_MI355X
// Same keys and defaults: item_type, GNSS-SDR.internal_fs_sps (2048000), doppler_max (5000,
// FLAGS_doppler_max over it), coherent_integration_time_ms (1), tong_init_val (1), tong_max_val
// (2), tong_max_dwells (tong_max_val + 1), AcquisitionMonitor.enable_monitor,
// <role><channel>.pfa and <role>.pfa.  dump is read and not mirrored.
//
// PcpsTongAcquisitionAdapterMI355X holds what this adapter and the Galileo E1 one
// (galileo_e1_pcps_tong_ambiguous_acquisition_mi355x.h) have word for word in common in the
// reference: the pass-through calls, set_threshold and calculate_threshold.
#ifndef GSDR_HOST_GPS_L1_CA_PCPS_TONG_ACQUISITION_MI355X_H
#define GSDR_HOST_GPS_L1_CA_PCPS_TONG_ACQUISITION_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_interface.h"
#include "configuration.h"
#include "pcps_tong_acquisition_mi355x.h"

class PcpsTongAcquisitionAdapterMI355X : public AcquisitionInterface
{
public:
    std::string role() override { return role_; }
    size_t item_size() override { return item_size_; }

    void set_gnss_synchro(Gnss_Synchro* gnss_synchro) override;
    void set_channel(unsigned int channel) override;
    // the block publishes its events itself; the reference's adapters keep no FSM either
    void set_channel_fsm(std::weak_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = std::move(channel_fsm); }
    void set_threshold(float threshold) override;
    void set_doppler_max(unsigned int doppler_max) override;
    void set_doppler_step(unsigned int doppler_step) override;
    void init() override { acquisition_->init(); }
    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return static_cast<signed int>(acquisition_->mag()); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override;
    void set_resampler_latency(uint32_t latency_samples __attribute__((unused))) override {}
    // the exponential quantile with lambda = vector_length over vector_length * bins cells
    float calculate_threshold(float pfa) const;

    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_tong_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int doppler_max() const { return doppler_max_; }
    unsigned int tong_init_val() const { return tong_init_val_; }
    unsigned int tong_max_val() const { return tong_max_val_; }
    unsigned int tong_max_dwells() const { return tong_max_dwells_; }
    float threshold() const { return threshold_; }

protected:
    // the keys both adapters read alike; default_fs is GNSS-SDR.internal_fs_hz's default and
    // default_ms coherent_integration_time_ms's
    PcpsTongAcquisitionAdapterMI355X(const ConfigurationInterface* configuration, const std::string& role,
        int64_t default_fs, int default_ms);
    // the block for items of vector_length_ samples, once the adapter has its lengths
    void make_block(int samples_per_ms, unsigned int in_streams, unsigned int out_streams, int device);

    const ConfigurationInterface* configuration_;
    std::unique_ptr<pcps_tong_acquisition_mi355x> acquisition_;
    std::weak_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_{nullptr};
    std::vector<std::complex<float>> code_;
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
    unsigned int tong_init_val_;
    unsigned int tong_max_val_;
    unsigned int tong_max_dwells_;
    bool dump_;
    bool enable_monitor_output_;
};

class GpsL1CaPcpsTongAcquisitionMI355X : public PcpsTongAcquisitionAdapterMI355X
{
public:
    GpsL1CaPcpsTongAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "GPS_L1_CA_PCPS_Tong_Acquisition_MI355X"; }
    // :189-205: the code period repeated coherent_integration_time_ms times
    void set_local_code() override;
};

#endif
