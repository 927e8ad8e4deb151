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
// (galileo_e1_pcps_tong_ambiguous_acquisition_mi355x.h) have in common beyond
// acquisition_item_adapter_mi355x.h: the Tong keys, the block and calculate_threshold.
#ifndef GSDR_HOST_GPS_L1_CA_PCPS_TONG_ACQUISITION_MI355X_H
#define GSDR_HOST_GPS_L1_CA_PCPS_TONG_ACQUISITION_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_item_adapter_mi355x.h"
#include "pcps_tong_acquisition_mi355x.h"

class PcpsTongAcquisitionAdapterMI355X : public AcquisitionItemAdapterMI355X
{
public:
    // the exponential quantile with lambda = vector_length over vector_length * bins cells
    float calculate_threshold(float pfa) const override;

    // the gr::block the reference connects behind its stream_to_vector (get_right_block)
    pcps_tong_acquisition_mi355x* get_block() { return acquisition_.get(); }
    unsigned int tong_init_val() const { return tong_init_val_; }
    unsigned int tong_max_val() const { return tong_max_val_; }
    unsigned int tong_max_dwells() const { return tong_max_dwells_; }

protected:
    // the keys both adapters read alike; default_fs is GNSS-SDR.internal_fs_hz's default and
    // default_ms coherent_integration_time_ms's
    PcpsTongAcquisitionAdapterMI355X(const ConfigurationInterface* configuration, const std::string& role,
        int64_t default_fs, int default_ms);
    // the block for items of vector_length_ samples, once the adapter has its lengths
    void make_block(int samples_per_ms, unsigned int in_streams, unsigned int out_streams, int device);

    std::unique_ptr<pcps_tong_acquisition_mi355x> acquisition_;
    std::vector<std::complex<float>> code_;
    unsigned int tong_init_val_;
    unsigned int tong_max_val_;
    unsigned int tong_max_dwells_;
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
