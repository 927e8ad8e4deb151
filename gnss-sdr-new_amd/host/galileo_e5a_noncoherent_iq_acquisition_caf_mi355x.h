// The Galileo E5a non-coherent IQ acquisition adapter with CAF filter on the MI355X engine: the
// counterpart of GalileoE5aNoncoherentIQAcquisitionCaf (src/algorithms/acquisition/adapters/
// galileo_e5a_noncoherent_iq_acquisition_caf.{h,cc}), selected in a .conf with
//   Acquisition_5X.implementation=Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_MI355X
// Same keys and defaults: item_type, GNSS-SDR.internal_fs_sps (32000000), doppler_max (5000,
// FLAGS_doppler_max over it), CAF_window_hz (0), Zero_padding (0),
// coherent_integration_time_ms (1, capped at 3; 2 with Zero_padding > 0: 1 ms of code and 1 ms
// of zeros), max_dwells (1), bit_transition_flag (false), Channel.signal (5X: both components),
// AcquisitionMonitor.enable_monitor, <role><channel>.pfa and <role>.pfa.  dump is read and not
// mirrored.
//
// The E5a primary codes are not part of this repository.  The block factory reads them from the
// file <role>.e5a_code_table names, or else the environment variable GSDR_GALILEO_E5A_CODES
// (gnss_replicas.h documents the layout), and refuses the block without a readable table of the
// right size.
#ifndef GSDR_HOST_GALILEO_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_MI355X_H
#define GSDR_HOST_GALILEO_E5A_NONCOHERENT_IQ_ACQUISITION_CAF_MI355X_H

#include <complex>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_item_adapter_mi355x.h"
#include "galileo_e5a_noncoherent_iq_acquisition_caf_block_mi355x.h"

class GalileoE5aNoncoherentIQAcquisitionCafMI355X : public AcquisitionItemAdapterMI355X
{
public:
    GalileoE5aNoncoherentIQAcquisitionCafMI355X(const ConfigurationInterface* configuration, const std::string& role,
        unsigned int in_streams, unsigned int out_streams, int device = 0);

    // The table the role's key or the environment names, loaded for the replica generator;
    // throws std::invalid_argument with the reason where there is none to load.
    static void load_code_table(const ConfigurationInterface* configuration, const std::string& role);

    std::string implementation() override { return "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_MI355X"; }

    // :212-262: the code period tiled coherent_integration_time_ms times, or followed by zeros
    void set_local_code() override;
    // the exponential quantile with lambda = vector_length over vector_length * bins cells (:274-291)
    float calculate_threshold(float pfa) const override;

    // the gr::block the reference connects (get_right_block)
    galileo_e5a_noncoherentIQ_acquisition_caf_mi355x* get_block() { return acquisition_.get(); }
    unsigned int max_dwells() const { return max_dwells_; }
    int CAF_window_hz() const { return CAF_window_hz_; }
    int zero_padding() const { return Zero_padding; }
    bool bit_transition_flag() const { return bit_transition_flag_; }
    bool both_signal_components_flag() const { return both_signal_components; }

private:
    std::unique_ptr<galileo_e5a_noncoherentIQ_acquisition_caf_mi355x> acquisition_;
    std::vector<std::complex<float>> codeI_, codeQ_;
    int Zero_padding;
    int CAF_window_hz_;
    unsigned int max_dwells_;
    bool bit_transition_flag_;
    bool both_signal_components{false};
};

#endif
