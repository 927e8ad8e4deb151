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

#include "acquisition_item_adapter_mi355x.h"
#include "pcps_pair_acquisition_mi355x.h"

// What the two adapters share beyond acquisition_item_adapter_mi355x.h: their keys and the block.
class GalileoE1PairAcquisitionMI355X : public AcquisitionItemAdapterMI355X
{
public:
    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_pair_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int max_dwells() const { return max_dwells_; }

protected:
    GalileoE1PairAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device, Pair_Acq_Conf::Policy policy);

    std::unique_ptr<pcps_pair_acquisition_mi355x> acquisition_;
    unsigned int max_dwells_;
};

class GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X : public GalileoE1PairAcquisitionMI355X
{
public:
    GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_MI355X"; }
    void set_threshold(float threshold) override;
    void set_local_code() override;
    // galileo_e1_pcps_cccwsr_ambiguous_acquisition.cc:219-225: not implemented there
    float calculate_threshold(float pfa __attribute__((unused))) const override { return 0.0F; }

private:
    std::vector<std::complex<float>> code_data_, code_pilot_;
};

class GalileoE1Pcps8msAmbiguousAcquisitionMI355X : public GalileoE1PairAcquisitionMI355X
{
public:
    GalileoE1Pcps8msAmbiguousAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_MI355X"; }
    void set_local_code() override;
    void stop_acquisition() override;
    float calculate_threshold(float pfa) const override;

private:
    std::vector<std::complex<float>> code_;
};

#endif
