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

#include "acquisition_item_adapter_mi355x.h"
#include "pcps_quicksync_acquisition_mi355x.h"

class GpsL1CaPcpsQuickSyncAcquisitionMI355X : public AcquisitionItemAdapterMI355X
{
public:
    GpsL1CaPcpsQuickSyncAcquisitionMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);

    std::string implementation() override { return "GPS_L1_CA_PCPS_QuickSync_Acquisition_MI355X"; }
    void set_local_code() override;
    float calculate_threshold(float pfa) const override;

    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_quicksync_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int folding_factor() const { return folding_factor_; }
    unsigned int max_dwells() const { return max_dwells_; }
    bool bit_transition_flag() const { return bit_transition_flag_; }

private:
    std::unique_ptr<pcps_quicksync_acquisition_mi355x> acquisition_;
    std::vector<std::complex<float>> code_;
    unsigned int folding_factor_;
    unsigned int max_dwells_;
    bool bit_transition_flag_;
};

#endif
