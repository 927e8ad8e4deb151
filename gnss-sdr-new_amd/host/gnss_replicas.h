// Code replica generators used on the acquisition / tracking hot path:
// GPS L1 C/A (src/algorithms/libs/gps_sdr_signal_replica.cc:25-176),
// Galileo E1 OS (src/algorithms/libs/galileo_e1_signal_replica.cc:29-233), Galileo E5a
// (src/algorithms/libs/galileo_e5_signal_replica.cc:31-124) and
// BeiDou B1I (src/algorithms/libs/beidou_b1i_signal_replica.cc:26-176).
#ifndef GSDR_HOST_GNSS_REPLICAS_H
#define GSDR_HOST_GNSS_REPLICAS_H

#include <complex>
#include <cstdint>
#include <string>
#include <vector>

// +1 / -1 chips of GPS L1 C/A for PRN 1-32 and SBAS 120-138 (empty on a bad PRN).
std::vector<int32_t> gps_l1_ca_code_gen_int(int32_t prn, uint32_t chip_shift = 0);
// float chips, one sample per chip (tracking replica, :104-115)
std::vector<float> gps_l1_ca_code_gen_float(int32_t prn, uint32_t chip_shift = 0);
// (0, +-1) chips (:118-131)
std::vector<std::complex<float>> gps_l1_ca_code_gen_complex(int32_t prn, uint32_t chip_shift = 0);
// sampled at fs with the reference's float index arithmetic (:136-176)
std::vector<std::complex<float>> gps_l1_ca_code_gen_complex_sampled(uint32_t prn, int32_t sampling_freq,
    uint32_t chip_shift = 0);

// ---- Galileo E1 (E1-B data "1B", E1-C pilot "1C") ----
// The ICD primary memory codes (Galileo OS SIS ICD Annex C, 50 PRNs x 4092 chips)
// are data: the bit-packed table gsdr/data/galileo_e1_codes.bin is assembled into
// the library (galileo_e1_codes.cc).  signal: "1B" or "1C".
// galileo_e1_code_gen_int (:29-58): +1 / -1 chips (hex_to_binary_converter: bit 0 -> +1)
std::vector<int32_t> galileo_e1_code_gen_int(const char* signal, int32_t prn);
// galileo_e1_code_gen_sinboc11_float (:100-111): tracking replica, 2 samples/chip (8184 floats)
std::vector<float> galileo_e1_code_gen_sinboc11_float(const char* signal, uint32_t prn);
// galileo_e1_code_gen_float_sampled (:146-210): sinBOC(1,1) (cboc false) or CBOC(6,1,1/11)
// sampled at fs (resampler of gnss_signal_replica.cc:257-272), optionally with the
// E1-C secondary code (25 primary periods)
std::vector<float> galileo_e1_code_gen_float_sampled(const char* signal, bool cboc, uint32_t prn, int32_t sampling_freq,
    uint32_t chip_shift = 0, bool secondary_flag = false);
// galileo_e1_code_gen_complex_sampled (:213-233): the same as real part, imaginary 0
std::vector<std::complex<float>> galileo_e1_code_gen_complex_sampled(const char* signal, bool cboc, uint32_t prn,
    int32_t sampling_freq, uint32_t chip_shift = 0, bool secondary_flag = false);

// ---- Galileo E5a (E5a-I data "5I", E5a-Q pilot "5Q", both "5X") ----
// The primary codes (Galileo OS SIS ICD Annex C: 50 PRNs x 10230 chips per component) are
// data the user supplies at run time; the repository ships no table.  The file holds 100 rows
// of 10230 bits, PRN 1-50 of E5a-I and then PRN 1-50 of E5a-Q, each row MSB first and padded
// to kGalileoE5aRowBytes bytes; a set bit is the chip -1 (hex_to_binary_converter: bit 0 -> +1).
constexpr uint32_t kGalileoE5aCodeLengthChips = 10230;
constexpr uint32_t kGalileoE5aRowBytes = 1279;
constexpr size_t kGalileoE5aTableBytes = 100 * static_cast<size_t>(kGalileoE5aRowBytes);
// Reads the table for the generators below; false, with the reason in *error, unless the file
// can be read and has exactly kGalileoE5aTableBytes bytes (the table in effect then stays).
bool galileo_e5a_load_code_table(const std::string& path, std::string* error = nullptr);
bool galileo_e5a_code_table_loaded();
// galileo_e5_a_code_gen_complex_primary (galileo_e5_signal_replica.cc:31-96): one sample per
// chip; "5I" and "5Q" real-valued rows, "5X" I + jQ.  Empty on a bad PRN or signal, or
// without a table.
std::vector<std::complex<float>> galileo_e5_a_code_gen_complex_primary(int32_t prn, const char* signal);
// galileo_e5_a_code_gen_complex_sampled (:99-124): dest[0, fs / 1000) gets one code period
// sampled at fs with the float resampler the E1 path has, circularly delayed by chip_shift
// chips; false (dest untouched) where the primary code is empty or dest is too short.
bool galileo_e5_a_code_gen_complex_sampled(std::vector<std::complex<float>>& dest, uint32_t prn, const char* signal,
    int32_t sampling_freq, uint32_t chip_shift = 0);

// The E5a-Q secondary codes (Galileo OS SIS ICD: one 100-chip code per PRN, the reference's
// GALILEO_E5A_Q_SECONDARY_CODE, Galileo_E5a.h:3585) are user data as well, needed by pilot
// tracking alone: 50 rows of 100 bits, PRN 1-50, each row MSB first and padded to
// kGalileoE5aSecondaryRowBytes bytes; a set bit is the character '1'.  Same conventions and
// refusals as the primary table.
constexpr uint32_t kGalileoE5aQSecondaryLength = 100;
constexpr uint32_t kGalileoE5aSecondaryRowBytes = 13;
constexpr size_t kGalileoE5aSecondaryTableBytes = 50 * static_cast<size_t>(kGalileoE5aSecondaryRowBytes);
bool galileo_e5a_load_secondary_table(const std::string& path, std::string* error = nullptr);
bool galileo_e5a_secondary_table_loaded();
// the PRN's E5a-Q secondary code as 100 characters '0' / '1'; empty on a bad PRN or without a table
std::string galileo_e5a_q_secondary_code(int32_t prn);
// The replicas of start_tracking for "5X" (dll_pll_veml_tracking.cc:696-719): pilot tracking
// takes the E5a-Q chips as tracking code and the E5a-I chips as data code, data tracking the
// E5a-I chips alone.  False where the primary code is missing.
bool galileo_e5a_tracking_codes(int32_t prn, bool track_pilot, std::vector<float>& code, std::vector<float>& data_code);

// ---- BeiDou B1I ----
// beidou_b1i_code_gen_int (:26-106): +1 / -1 chips of PRN 1-63 (2046 chips; empty on a bad PRN)
std::vector<int32_t> beidou_b1i_code_gen_int(int32_t prn, uint32_t chip_shift = 0);
// beidou_b1i_code_gen_float (:109-120): tracking replica, one sample per chip
std::vector<float> beidou_b1i_code_gen_float(int32_t prn, uint32_t chip_shift = 0);
// beidou_b1i_code_gen_complex_sampled (:137-176): (+-1, 0) sampled at fs
std::vector<std::complex<float>> beidou_b1i_code_gen_complex_sampled(uint32_t prn, int32_t sampling_freq,
    uint32_t chip_shift = 0);

#endif
