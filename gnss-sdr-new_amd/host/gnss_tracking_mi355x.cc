#include "gnss_tracking_mi355x.h"

#include <cmath>
#include <cstdlib>
#include <iostream>
#include <stdexcept>

#include "gnss_replicas.h"

namespace
{
constexpr double GPS_L1_CA_CODE_RATE_CPS = 1.023e6;  // GPS_L1_CA.h
constexpr double GPS_L1_CA_CODE_LENGTH_CHIPS = 1023.0;
constexpr double GALILEO_E1_CODE_CHIP_RATE_CPS = 1.023e6;  // Galileo_E1.h
constexpr double GALILEO_E1_B_CODE_LENGTH_CHIPS = 4092.0;
constexpr double BEIDOU_B1I_CODE_RATE_CPS = 2.046e6;  // Beidou_B1I.h
constexpr double BEIDOU_B1I_CODE_LENGTH_CHIPS = 2046.0;
constexpr double GALILEO_E5A_CODE_CHIP_RATE_CPS = 1.023e7;  // Galileo_E5a.h
constexpr double GALILEO_E5A_CODE_LENGTH_CHIPS = 10230.0;
constexpr int GALILEO_E5A_I_SECONDARY_CODE_LENGTH = 20;
}  // namespace

void DllPllTrackingAdapterMI355X::make_block(const ConfigurationInterface* configuration, int32_t signal, int device)
{
    item_size_ = trk_params_.item_type == "cshort" ? 4 : (trk_params_.item_type == "cbyte" ? 2 : 8);
    // pooled by default: every channel of the signal on this GPU in one engine
    // handle over the device ring, one launch per <role>.mi355x_pool_batch
    // correlation lengths for all its channels, instead of a per-channel block's
    // synchronous H2D + launch + D2H per general_work call
    pooled_ = configuration->property(role_ + ".mi355x_pool", true);
    if (!pooled_)
        {
            std::cerr << role_ << ": " << implementation_
                      << " built per channel (" << role_ << ".mi355x_pool=false): one synchronous device round trip "
                      << "per general_work call, about 10x the pooled block's cost\n";
            tracking_ = std::make_unique<dll_pll_veml_tracking_mi355x>(trk_params_, signal, device);
            return;
        }
    // the role's suffix names the signal's channel count key (Tracking_1C -> Channels_1C.count)
    const std::string sig = role_.size() >= 2 ? role_.substr(role_.size() - 2) : std::string("1C");
    const int count = configuration->property("Channels_" + sig + ".count", 32);
    const int slots = configuration->property(role_ + ".mi355x_pool_channels", count > 0 ? count : 32);
    const int window = configuration->property(role_ + ".mi355x_pool_window",
        static_cast<int>(SharedTrackingPool::kDefaultWindowCalls));
    const int batch = configuration->property(role_ + ".mi355x_pool_batch",
        static_cast<int>(SharedTrackingPool::kDefaultBatchCalls));
    // the input stream's shared device ring: roles naming the same ring read the same
    // conditioner output (a multi-constellation receiver on one front end names one
    // ring for all its signals, so the stream crosses PCIe once); default: the role's own
    const std::string ring = configuration->property(role_ + ".mi355x_ring", role_);
    tracking_ = std::make_unique<dll_pll_veml_tracking_pool_mi355x>(trk_params_, signal,
        static_cast<uint32_t>(slots > 0 ? slots : 32), device, role_, static_cast<uint32_t>(window),
        static_cast<uint32_t>(batch), ring);
}

// gps_l1_ca_dll_pll_tracking.cc:34-91
GpsL1CaDllPllTrackingMI355X::GpsL1CaDllPllTrackingMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : DllPllTrackingAdapterMI355X(role, "GPS_L1_CA_DLL_PLL_Tracking_MI355X")
{
    (void)in_streams;
    (void)out_streams;
    trk_params_.SetFromConfiguration(configuration, role);
    trk_params_.vector_length = static_cast<uint32_t>(
        std::round(trk_params_.fs_in / (GPS_L1_CA_CODE_RATE_CPS / GPS_L1_CA_CODE_LENGTH_CHIPS)));
    if (trk_params_.extend_correlation_symbols < 1) trk_params_.extend_correlation_symbols = 1;
    if (trk_params_.extend_correlation_symbols > 20) trk_params_.extend_correlation_symbols = 20;
    // GPS L1 C/A has no pilot: data tracking (:52-57)
    trk_params_.track_pilot = false;
    trk_params_.system = 'G';
    trk_params_.signal[0] = '1';
    trk_params_.signal[1] = 'C';
    make_block(configuration, GSDR_SIGNAL_GPS_1C, device);
}

// gps_l1_ca_kf_tracking.cc:34-93
GpsL1CaKfTrackingMI355X::GpsL1CaKfTrackingMI355X(const ConfigurationInterface* configuration, const std::string& role,
    unsigned int in_streams, unsigned int out_streams, int device)
    : DllPllTrackingAdapterMI355X(role, "GPS_L1_CA_KF_Tracking_MI355X")
{
    (void)in_streams;
    (void)out_streams;
    Kf_Conf kf_params;
    kf_params.SetFromConfiguration(configuration, role);
    trk_params_ = kf_params;  // the Dll_Pll_Conf part carries kf and the Kalman values
    trk_params_.vector_length = static_cast<uint32_t>(
        std::round(trk_params_.fs_in / (GPS_L1_CA_CODE_RATE_CPS / GPS_L1_CA_CODE_LENGTH_CHIPS)));
    if (trk_params_.extend_correlation_symbols < 1)
        {
            trk_params_.extend_correlation_symbols = 1;
            std::cout << "WARNING: GPS L1 C/A. extend_correlation_symbols must be bigger than 1. Coherent integration has "
                         "been set to 1 symbol (1 ms)\n";
        }
    else if (trk_params_.extend_correlation_symbols > 20)
        {
            trk_params_.extend_correlation_symbols = 20;
            std::cout << "WARNING: GPS L1 C/A. extend_correlation_symbols must be lower than 21. Coherent integration has "
                         "been set to 20 symbols (20 ms)\n";
        }
    trk_params_.track_pilot = false;
    if (trk_params_.high_dyn)
        throw std::invalid_argument(role + ": the Kalman loop has no high-dynamics branch on this engine (high_dyn=true)");
    trk_params_.system = 'G';
    trk_params_.signal[0] = '1';
    trk_params_.signal[1] = 'C';
    make_block(configuration, GSDR_SIGNAL_GPS_1C, device);
}

// galileo_e1_dll_pll_veml_tracking.cc:34-75: extended integration only when
// tracking the pilot
GalileoE1DllPllVemlTrackingMI355X::GalileoE1DllPllVemlTrackingMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : DllPllTrackingAdapterMI355X(role, "Galileo_E1_DLL_PLL_VEML_Tracking_MI355X")
{
    (void)in_streams;
    (void)out_streams;
    trk_params_.SetFromConfiguration(configuration, role);
    if (trk_params_.extend_correlation_symbols < 1)
        trk_params_.extend_correlation_symbols = 1;
    else if (!trk_params_.track_pilot && trk_params_.extend_correlation_symbols > 1)
        trk_params_.extend_correlation_symbols = 1;
    trk_params_.vector_length = static_cast<uint32_t>(
        std::round(trk_params_.fs_in / (GALILEO_E1_CODE_CHIP_RATE_CPS / GALILEO_E1_B_CODE_LENGTH_CHIPS)));
    trk_params_.system = 'E';
    trk_params_.signal[0] = '1';
    trk_params_.signal[1] = 'B';
    make_block(configuration, GSDR_SIGNAL_GAL_1B, device);
}

// galileo_e5a_dll_pll_tracking.cc:33-82
GalileoE5aDllPllTrackingMI355X::GalileoE5aDllPllTrackingMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : DllPllTrackingAdapterMI355X(role, "Galileo_E5a_DLL_PLL_Tracking_MI355X")
{
    (void)in_streams;
    (void)out_streams;
    trk_params_.SetFromConfiguration(configuration, role);
    trk_params_.vector_length = static_cast<uint32_t>(
        std::round(trk_params_.fs_in / (GALILEO_E5A_CODE_CHIP_RATE_CPS / GALILEO_E5A_CODE_LENGTH_CHIPS)));
    if (trk_params_.extend_correlation_symbols < 1)
        {
            trk_params_.extend_correlation_symbols = 1;
            std::cout << "WARNING: Galileo E5a. extend_correlation_symbols must be bigger than 0. Coherent integration "
                         "has been set to 1 symbol (1 ms)\n";
        }
    else if (!trk_params_.track_pilot && trk_params_.extend_correlation_symbols > GALILEO_E5A_I_SECONDARY_CODE_LENGTH)
        {
            trk_params_.extend_correlation_symbols = GALILEO_E5A_I_SECONDARY_CODE_LENGTH;
            std::cout << "WARNING: Galileo E5a. extend_correlation_symbols must be lower than 21 when tracking the data "
                         "component. Coherent integration has been set to 20 symbols (20 ms)\n";
        }
    if (trk_params_.extend_correlation_symbols > 1 &&
        (trk_params_.pll_bw_narrow_hz > trk_params_.pll_bw_hz || trk_params_.dll_bw_narrow_hz > trk_params_.dll_bw_hz))
        std::cout << "WARNING: Galileo E5a. PLL or DLL narrow tracking bandwidth is higher than wide tracking one\n";
    trk_params_.system = 'E';
    trk_params_.signal[0] = '5';
    trk_params_.signal[1] = 'X';
    // the user's code files (the repository ships none)
    std::string why;
    const char* env = std::getenv("GSDR_GALILEO_E5A_CODES");
    const std::string codes = configuration->property(role + ".e5a_code_table", std::string(env ? env : ""));
    if (codes.empty())
        throw std::invalid_argument(role + ": the Galileo E5a primary codes are not shipped: name a code table with " + role +
                                    ".e5a_code_table or GSDR_GALILEO_E5A_CODES (layout: gnss_replicas.h)");
    if (!galileo_e5a_load_code_table(codes, &why)) throw std::invalid_argument(role + ": " + why);
    if (trk_params_.track_pilot)
        {
            env = std::getenv("GSDR_GALILEO_E5A_SECONDARY_CODES");
            const std::string sec = configuration->property(role + ".e5a_secondary_code_table", std::string(env ? env : ""));
            if (sec.empty())
                throw std::invalid_argument(role + ": pilot tracking needs the E5a-Q secondary codes, which are not shipped: "
                                                   "name a table with " + role + ".e5a_secondary_code_table or "
                                                   "GSDR_GALILEO_E5A_SECONDARY_CODES (layout: gnss_replicas.h)");
            if (!galileo_e5a_load_secondary_table(sec, &why)) throw std::invalid_argument(role + ": " + why);
        }
    make_block(configuration, GSDR_SIGNAL_GAL_5X, device);
}

// beidou_b1i_dll_pll_tracking.cc:34-90
BeidouB1iDllPllTrackingMI355X::BeidouB1iDllPllTrackingMI355X(const ConfigurationInterface* configuration,
    const std::string& role, unsigned int in_streams, unsigned int out_streams, int device)
    : DllPllTrackingAdapterMI355X(role, "BEIDOU_B1I_DLL_PLL_Tracking_MI355X")
{
    (void)in_streams;
    (void)out_streams;
    trk_params_.SetFromConfiguration(configuration, role);
    trk_params_.vector_length = static_cast<uint32_t>(
        std::round(trk_params_.fs_in / (BEIDOU_B1I_CODE_RATE_CPS / BEIDOU_B1I_CODE_LENGTH_CHIPS)));
    if (trk_params_.extend_correlation_symbols < 1) trk_params_.extend_correlation_symbols = 1;
    if (trk_params_.extend_correlation_symbols > 20) trk_params_.extend_correlation_symbols = 20;
    trk_params_.track_pilot = false;
    trk_params_.system = 'C';
    trk_params_.signal[0] = 'B';
    trk_params_.signal[1] = '1';
    make_block(configuration, GSDR_SIGNAL_BDS_B1, device);
}
