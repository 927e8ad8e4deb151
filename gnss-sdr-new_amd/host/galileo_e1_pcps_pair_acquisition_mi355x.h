// The two Galileo E1 paired-code acquisition adapters on the MI355X engine: the
// counterparts of GalileoE1PcpsCccwsrAmbiguousAcquisition and
// GalileoE1Pcps8msAmbiguousAcquisition (src/algorithms/acquisition/adapters/
// galileo_e1_pcps_cccwsr_ambiguous_acquisition.{h,cc},
// galileo_e1_pcps_8ms_ambiguous_acquisition.{h,cc}), selected in a .conf with
//   Acquisition_1B.implementation=Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_MI355X
//   Acquisition_1B.implementation=Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_MI355X
// Same keys and defaults: item_type, GNSS-SDR.internal_fs_sps (4000000), doppler_max (5000,
// FLAGS_doppler_max over it), coherent_integration_time_ms (4, rounded down to a multiple of
// 4), max_dwells (1), Acquisition<channel>.cboc (false); the 8 ms adapter also <role><channel>.pfa
// and <role>.pfa.  dump is read and not mirrored (pcps_pair_acquisition_mi355x.h).
#ifndef GSDR_HOST_GALILEO_E1_PCPS_PAIR_ACQUISITION_MI355X_H
#define GSDR_HOST_GALILEO_E1_PCPS_PAIR_ACQUISITION_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_interface.h"
#include "configuration.h"
#include "pcps_pair_acquisition_mi355x.h"

// What the two adapters share: the keys, the block and the pass-through setters.
class GalileoE1PairAcquisitionMI355X : public AcquisitionInterface
{
public:
    std::string role() override { return role_; }
    size_t item_size() override { return item_size_; }

    void set_gnss_synchro(Gnss_Synchro* gnss_synchro) override;
    void set_channel(unsigned int channel) override;
    // the block publishes its events itself; the reference's adapters keep no FSM either
    void set_channel_fsm(std::weak_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = std::move(channel_fsm); }
    void set_doppler_max(unsigned int doppler_max) override;
    void set_doppler_step(unsigned int doppler_step) override;
    void init() override { acquisition_->init(); }
    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return static_cast<signed int>(acquisition_->mag()); }
    void reset() override { acquisition_->set_active(true); }
    void set_resampler_latency(uint32_t latency_samples __attribute__((unused))) override {}

    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_pair_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int vector_length() const { return vector_length_; }
    unsigned int code_length() const { return code_length_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    unsigned int doppler_max() const { return doppler_max_; }
    float threshold() const { return threshold_; }

protected:
    GalileoE1PairAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device, Pair_Acq_Conf::Policy policy);

    const ConfigurationInterface* configuration_;
    std::unique_ptr<pcps_pair_acquisition_mi355x> acquisition_;
    std::weak_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_{nullptr};
    std::string item_type_;
    std::string dump_filename_;
    std::string role_;
    int64_t fs_in_;
    size_t item_size_;
    float threshold_{0.0F};
    unsigned int doppler_max_;
    unsigned int vector_length_;
    unsigned int code_length_;
    unsigned int channel_{0};
    unsigned int doppler_step_{0};
    unsigned int sampled_ms_;
    unsigned int max_dwells_;
    bool dump_;
};

class GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X : public GalileoE1PairAcquisitionMI355X
{
public:
    GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_MI355X"; }
    void set_threshold(float threshold) override;
    void set_local_code() override;
    void stop_acquisition() override;
    // galileo_e1_pcps_cccwsr_ambiguous_acquisition.cc:219-225: not implemented there
    float calculate_threshold(float pfa __attribute__((unused))) const { return 0.0F; }

private:
    std::vector<std::complex<float>> code_data_, code_pilot_;
};

class GalileoE1Pcps8msAmbiguousAcquisitionMI355X : public GalileoE1PairAcquisitionMI355X
{
public:
    GalileoE1Pcps8msAmbiguousAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_MI355X"; }
    void set_threshold(float threshold) override;
    void set_local_code() override;
    void stop_acquisition() override;
    float calculate_threshold(float pfa) const;

private:
    std::vector<std::complex<float>> code_;
};

#endif
