// The acquisition resampler of GNSS-SDR.use_acquisition_resampler on the device
// ring path: one decimating FIR (gsdr_decim, csrc/decim.hip) per signal and input
// stream, shared by every acquisition service of that signal, exactly as the
// reference flowgraph shares one gr::filter::fir_filter_ccf per map_key = signal
// string + RF channel (gnss_flowgraph.cc:1069-1113).
//
// The decimation is the one Acq_Conf derived (resampler_ratio,
// acq_conf.cc:93-111), so the decimated ring runs at the rate the consumer's own
// replicas and block length were computed for (resampled_fs); the taps are the
// flowgraph's low_pass(1, fs, fs_d / 2.1, fs_d / 2), and latency() is what the
// flowgraph hands to set_resampler_latency ((taps - 1) / 2, :1112).
//
// A resampler is built wherever Acq_Conf asks for one
// (use_automatic_resampler && resampler_ratio > 1).  That includes BeiDou B1I,
// whose adapter passes 10 Msps as opt_freq: the reference flowgraph builds no FIR
// for evBDS_B1 (:1061-1064) although its Acq_Conf samples the replica at
// resampled_fs -- see DESIGN.md.
#ifndef GSDR_HOST_ACQ_RESAMPLER_H
#define GSDR_HOST_ACQ_RESAMPLER_H

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "acq_conf.h"
#include "gsdr.h"

class AcqResampler
{
public:
    // the smallest window (decimated items) a shared decimated ring is created with
    static constexpr uint64_t kMinWindow = uint64_t(1) << 20;

    static bool wanted(const Acq_Conf& conf) { return conf.use_automatic_resampler && conf.resampler_ratio > 1.0F; }

    // The process's resampler of (device of `source`, ring_key, signal) -- the
    // reference's map_key -- reading `source`; nullptr when `conf` asks for none.
    // window_items: the longest window (decimated items) the consumer reads.  A
    // consumer whose source ring, decimation or window does not fit the existing
    // resampler gets one of its own.
    static std::shared_ptr<AcqResampler> get(gsdr_stream* source, const std::string& ring_key, const std::string& signal,
        const Acq_Conf& conf, uint64_t window_items);

    AcqResampler(gsdr_stream* source, const Acq_Conf& conf, uint64_t window_items);  // 2 x window positions
    ~AcqResampler();
    AcqResampler(const AcqResampler&) = delete;
    AcqResampler& operator=(const AcqResampler&) = delete;

    gsdr_stream* source() const { return d_source; }
    gsdr_stream* output() const { return d_output; }  // GSDR_ITEM_GR_COMPLEX at resampled_fs
    uint32_t decimation() const { return d_decimation; }
    uint32_t latency() const { return d_latency; }  // input samples, for set_resampler_latency
    uint64_t window() const { return d_window; }
    const std::vector<float>& taps() const { return d_taps; }

    // filters what the source holds since the last call (asynchronous, any thread);
    // returns the decimated ring's head; throws std::runtime_error on GSDR_E_*
    uint64_t advance();

private:
    gsdr_stream* d_source;
    gsdr_decim* d_decim{nullptr};
    gsdr_stream* d_output{nullptr};
    uint32_t d_decimation{1};
    uint32_t d_latency{0};
    uint64_t d_window;
    std::vector<float> d_taps;
};

#endif
