#include "gnss_block_factory_mi355x.h"

#include "beidou_b1i_pcps_acquisition_mi355x.h"
#include "galileo_e1_pcps_ambiguous_acquisition_mi355x.h"
#include "galileo_e1_pcps_pair_acquisition_mi355x.h"
#include "galileo_e1_pcps_tong_ambiguous_acquisition_mi355x.h"
#include "galileo_e5a_noncoherent_iq_acquisition_caf_mi355x.h"
#include "gnss_tracking_mi355x.h"
#include "gps_l1_ca_pcps_acquisition_fine_doppler_mi355x.h"
#include "gps_l1_ca_pcps_acquisition_mi355x.h"
#include "gps_l1_ca_pcps_quicksync_acquisition_mi355x.h"
#include "gps_l1_ca_pcps_tong_acquisition_mi355x.h"
#include "gsdr.h"

namespace gsdr_factory
{
int device_for_channel(const ConfigurationInterface* configuration, const std::string& role, int channel)
{
    const int pinned = configuration->property(role + ".device", -1);
    if (pinned >= 0) return pinned;
    int visible = 0;
    if (gsdr_device_count(&visible) != GSDR_OK || visible < 1) visible = 1;
    int g = configuration->property("GNSS-SDR.mi355x_devices", visible);
    if (g < 1 || g > visible) g = visible;
    return (channel < 0 ? 0 : channel) % g;
}

std::unique_ptr<AcquisitionInterface> GetAcqBlock(const ConfigurationInterface* configuration, const std::string& role,
    unsigned int in_streams, unsigned int out_streams, int channel)
{
    const std::string implementation = configuration->property(role + ".implementation", std::string("Wrong"));
    const int device = device_for_channel(configuration, role, channel);
    if (implementation == "GPS_L1_CA_PCPS_Acquisition_MI355X")
        return std::make_unique<GpsL1CaPcpsAcquisitionMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_MI355X")
        return std::make_unique<GpsL1CaPcpsAcquisitionFineDopplerMI355X>(configuration, role, in_streams, out_streams,
            device);
    if (implementation == "GPS_L1_CA_PCPS_QuickSync_Acquisition_MI355X")
        return std::make_unique<GpsL1CaPcpsQuickSyncAcquisitionMI355X>(configuration, role, in_streams, out_streams,
            device);
    if (implementation == "GPS_L1_CA_PCPS_Tong_Acquisition_MI355X")
        return std::make_unique<GpsL1CaPcpsTongAcquisitionMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_MI355X")
        return std::make_unique<GalileoE1PcpsTongAmbiguousAcquisitionMI355X>(configuration, role, in_streams,
            out_streams, device);
    if (implementation == "Galileo_E1_PCPS_Ambiguous_Acquisition_MI355X")
        return std::make_unique<GalileoE1PcpsAmbiguousAcquisitionMI355X>(configuration, role, in_streams, out_streams,
            device);
    if (implementation == "Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_MI355X")
        return std::make_unique<GalileoE1PcpsCccwsrAmbiguousAcquisitionMI355X>(configuration, role, in_streams,
            out_streams, device);
    if (implementation == "Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_MI355X")
        return std::make_unique<GalileoE1Pcps8msAmbiguousAcquisitionMI355X>(configuration, role, in_streams, out_streams,
            device);
    if (implementation == "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_MI355X")
        {
            // the E5a primary codes come from the user's table: no block without one (throws, with the reason)
            GalileoE5aNoncoherentIQAcquisitionCafMI355X::load_code_table(configuration, role);
            return std::make_unique<GalileoE5aNoncoherentIQAcquisitionCafMI355X>(configuration, role, in_streams,
                out_streams, device);
        }
    if (implementation == "BEIDOU_B1I_PCPS_Acquisition_MI355X")
        return std::make_unique<BeidouB1iPcpsAcquisitionMI355X>(configuration, role, in_streams, out_streams, device);
    return nullptr;
}

std::unique_ptr<TrackingInterface> GetTrkBlock(const ConfigurationInterface* configuration, const std::string& role,
    unsigned int in_streams, unsigned int out_streams, int channel)
{
    const std::string implementation = configuration->property(role + ".implementation", std::string("Wrong"));
    const int device = device_for_channel(configuration, role, channel);
    if (implementation == "GPS_L1_CA_DLL_PLL_Tracking_MI355X")
        return std::make_unique<GpsL1CaDllPllTrackingMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "GPS_L1_CA_KF_Tracking_MI355X")
        return std::make_unique<GpsL1CaKfTrackingMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "Galileo_E1_DLL_PLL_VEML_Tracking_MI355X")
        return std::make_unique<GalileoE1DllPllVemlTrackingMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "Galileo_E5a_DLL_PLL_Tracking_MI355X")
        return std::make_unique<GalileoE5aDllPllTrackingMI355X>(configuration, role, in_streams, out_streams, device);
    if (implementation == "BEIDOU_B1I_DLL_PLL_Tracking_MI355X")
        return std::make_unique<BeidouB1iDllPllTrackingMI355X>(configuration, role, in_streams, out_streams, device);
    return nullptr;
}

std::unique_ptr<AcquisitionService> GetAcqService(const ConfigurationInterface* configuration, const std::string& role,
    const std::string& signal, uint32_t max_requests, gsdr_stream* ring, const std::string& ring_key,
    uint32_t batch_blocks)
{
    // ms_per_code, chip rate and optimum acquisition rate of the signal's adapter
    Acq_Conf conf;
    double chip_rate, opt_freq;
    if (signal == "1C")
        conf.ms_per_code = 1, chip_rate = 1.023e6, opt_freq = 2000000.0;
    else if (signal == "1B")
        conf.ms_per_code = 4, chip_rate = 1.023e6, opt_freq = 2000000.0;
    else if (signal == "B1")
        conf.ms_per_code = 1, chip_rate = 2.046e6, opt_freq = 10e6;
    else
        return nullptr;
    conf.SetFromConfiguration(configuration, role, chip_rate, opt_freq);
    int device = 0;
    if (!ring || gsdr_stream_device(ring, &device) != GSDR_OK) return nullptr;
    auto svc = std::make_unique<AcquisitionService>(conf, max_requests, device, batch_blocks);
    if (AcqResampler::wanted(conf))
        {
            // two launches of batch_blocks blocks in flight on the decimated ring
            const uint64_t block = static_cast<uint64_t>(conf.sampled_ms * conf.samples_per_ms);
            svc->attach_resampler(AcqResampler::get(ring, ring_key, signal, conf, 4 * batch_blocks * block));
        }
    return svc;
}
}  // namespace gsdr_factory
