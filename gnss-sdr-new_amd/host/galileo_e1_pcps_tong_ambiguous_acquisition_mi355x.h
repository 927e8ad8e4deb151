// The Galileo E1 Tong acquisition adapter on the MI355X engine: the counterpart of
// GalileoE1PcpsTongAmbiguousAcquisition (src/algorithms/acquisition/adapters/
// galileo_e1_pcps_tong_ambiguous_acquisition.{h,cc}), selected in a .conf with
//   Acquisition_1B.implementation=Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_MI355X
// Same keys and defaults as the GPS adapter but GNSS-SDR.internal_fs_hz (4000000) and
// coherent_integration_time_ms (4, rounded down to a multiple of 4 as the reference rounds it,
// :67-73); items are code_length * (coherent_integration_time_ms / 4) samples, samples_per_ms
// code_length / 4 (:86-91); Acquisition<channel>.cboc (false) selects CBOC over sinBOC(1,1), under
// the reference's own key (:211-212: no role in it).
#ifndef GSDR_HOST_GALILEO_E1_PCPS_TONG_AMBIGUOUS_ACQUISITION_MI355X_H
#define GSDR_HOST_GALILEO_E1_PCPS_TONG_AMBIGUOUS_ACQUISITION_MI355X_H

#include "gps_l1_ca_pcps_tong_acquisition_mi355x.h"

class GalileoE1PcpsTongAmbiguousAcquisitionMI355X : public PcpsTongAcquisitionAdapterMI355X
{
public:
    GalileoE1PcpsTongAmbiguousAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);
    std::string implementation() override { return "Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_MI355X"; }
    // :207-230: the 4 ms code repeated coherent_integration_time_ms / 4 times
    void set_local_code() override;
};

#endif
