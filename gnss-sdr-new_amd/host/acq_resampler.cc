#include "acq_resampler.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <tuple>

std::shared_ptr<AcqResampler> AcqResampler::get(gsdr_stream* source, const std::string& ring_key,
    const std::string& signal, const Acq_Conf& conf, uint64_t window_items)
{
    if (!wanted(conf)) return nullptr;
    int device = 0;
    if (!source || gsdr_stream_device(source, &device) != GSDR_OK)
        throw std::invalid_argument("AcqResampler::get: no source ring");
    static std::mutex mu;
    static std::map<std::tuple<int, std::string, std::string>, std::weak_ptr<AcqResampler>> registry;
    std::lock_guard<std::mutex> lk(mu);
    auto& w = registry[std::make_tuple(device, ring_key, signal)];
    if (auto p = w.lock())
        {
            if (p->source() == source && p->decimation() == static_cast<uint32_t>(conf.resampler_ratio) &&
                p->window() >= window_items)
                return p;
            return std::make_shared<AcqResampler>(source, conf, window_items);  // its own
        }
    auto p = std::make_shared<AcqResampler>(source, conf, std::max(window_items, kMinWindow));
    w = p;
    return p;
}

AcqResampler::AcqResampler(gsdr_stream* source, const Acq_Conf& conf, uint64_t window_items)
    : d_source(source), d_window(window_items)
{
    if (!wanted(conf)) throw std::invalid_argument("AcqResampler: the configuration asks for no resampler");
    d_decimation = static_cast<uint32_t>(conf.resampler_ratio);
    // gnss_flowgraph.cc:1079-1087
    const double fs = static_cast<double>(conf.fs_in);
    const double fs_d = fs / static_cast<double>(d_decimation);
    d_taps.resize(4096);
    auto ntaps = static_cast<uint32_t>(d_taps.size());
    if (gsdr_firdes_low_pass(1.0, fs, fs_d / 2.1, fs_d / 2.0, d_taps.data(), &ntaps) != GSDR_OK)
        throw std::runtime_error(std::string("AcqResampler: ") + gsdr_last_error());
    d_taps.resize(ntaps);
    d_latency = (ntaps - 1) / 2;  // :1112
    if (gsdr_decim_create(source, d_decimation, d_taps.data(), ntaps, 2 * d_window, d_window, &d_decim) != GSDR_OK ||
        gsdr_decim_output(d_decim, &d_output) != GSDR_OK)
        {
            const std::string why = gsdr_last_error();
            gsdr_decim_destroy(d_decim);
            throw std::runtime_error("AcqResampler: " + why);
        }
}

AcqResampler::~AcqResampler() { gsdr_decim_destroy(d_decim); }

uint64_t AcqResampler::advance()
{
    uint64_t head = 0;
    if (gsdr_decim_advance(d_decim, &head) != GSDR_OK)
        throw std::runtime_error(std::string("AcqResampler::advance: ") + gsdr_last_error());
    return head;
}
