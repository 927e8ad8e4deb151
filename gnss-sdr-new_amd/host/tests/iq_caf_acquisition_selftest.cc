// Self-test driver of the Galileo E5a non-coherent IQ acquisition block with CAF filter
// (tests/test_host_iq_caf.py).
//
//   iq_caf_acquisition_selftest <file.conf> <iq.dat> <role> <prn> <threshold> <attempts> <ring 0|1> [items per call]
//
// Reads a GNSS-SDR style .conf (name=value lines, ';' comments), builds the block of <role>
// (Acquisition_5X) from it through the block factory -- which reads the E5a code table the
// .conf or the environment names -- and feeds it the gr_complex samples of iq.dat as items of the
// adapter's vector length through its state machine, `attempts` acquisitions one after the other
// (reset() after each event), offering `items per call` items (default 1) to every work() call.
// The satellite's signal is Channel.signal's.  With ring = 1 the samples are also pushed into a
// device ring and the block reads its items there.  Prints one JSON line: per attempt, for every
// work() call the state before it, the items it consumed, the event it published (0: none), the
// dwell count and statistic, the Gnss_Synchro acquisition fields after it and the monitor output,
// if the call produced one.
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "configuration.h"
#include "gnss_block_factory_mi355x.h"
#include "galileo_e5a_noncoherent_iq_acquisition_caf_mi355x.h"
#include "gsdr.h"

namespace
{
std::string trim(const std::string& s)
{
    const auto a = s.find_first_not_of(" \t\r\n");
    if (a == std::string::npos) return "";
    return s.substr(a, s.find_last_not_of(" \t\r\n") - a + 1);
}

bool read_conf(const std::string& path, InMemoryConfiguration& config)
{
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line))
        {
            line = trim(line.substr(0, line.find(';')));
            const auto eq = line.find('=');
            if (line.empty() || line[0] == '[' || eq == std::string::npos) continue;
            config.set_property(trim(line.substr(0, eq)), trim(line.substr(eq + 1)));
        }
    return true;
}

int report_error(const char* stage, const std::exception& e)
{
    std::string what = e.what();
    std::replace(what.begin(), what.end(), '"', '\'');
    std::cout << "{\"built\": " << (std::string(stage) == "built" ? "false" : "true, \"configured\": false")
              << ", \"error\": \"" << what << "\"}\n";
    return 1;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 8)
        {
            std::cerr << "usage: iq_caf_acquisition_selftest <file.conf> <iq.dat> <role> <prn> <threshold> <attempts> <ring> "
                         "[items per call]\n";
            return 2;
        }
    InMemoryConfiguration config;
    if (!read_conf(argv[1], config))
        {
            std::cerr << "cannot read " << argv[1] << '\n';
            return 2;
        }
    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    if (!f)
        {
            std::cerr << "cannot read " << argv[2] << '\n';
            return 2;
        }
    std::vector<std::complex<float>> x(static_cast<size_t>(f.tellg()) / sizeof(std::complex<float>));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(x.data()), static_cast<std::streamsize>(x.size() * sizeof(std::complex<float>)));
    const std::string role = argv[3];
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[4]));
    const float threshold = static_cast<float>(std::atof(argv[5]));
    const int attempts = std::atoi(argv[6]);
    const bool use_ring = std::atoi(argv[7]) != 0;
    const int per_call = argc > 8 ? std::max(1, std::atoi(argv[8])) : 1;

    std::unique_ptr<AcquisitionInterface> acq;
    try
        {
            acq = gsdr_factory::GetAcqBlock(&config, role, 1, 0, 0);
        }
    catch (const std::exception& e)
        {
            return report_error("built", e);
        }
    if (!acq)
        {
            std::cout << "{\"built\": false}\n";
            return 1;
        }
    auto* adapter = dynamic_cast<GalileoE5aNoncoherentIQAcquisitionCafMI355X*>(acq.get());
    if (!adapter)
        {
            std::cout << "{\"built\": true, \"implementation\": \"" << acq->implementation() << "\", \"iq_caf\": false}\n";
            return 1;
        }
    auto* block = adapter->get_block();
    Gnss_Synchro synchro;
    const std::string signal = config.property("Channel.signal", std::string("5X"));
    synchro.System = 'E';
    synchro.Signal[0] = signal.size() > 0 ? signal[0] : '5';
    synchro.Signal[1] = signal.size() > 1 ? signal[1] : 'X';
    synchro.PRN = prn;
    int event = 0;
    block->set_event_handler([&event](int e) { event = e; });
    // the Doppler grid before the threshold: the adapter's pfa threshold counts its rows
    try
        {
            acq->set_channel(0);
            acq->set_gnss_synchro(&synchro);
            acq->set_doppler_max(static_cast<unsigned int>(config.property(role + ".doppler_max", 5000)));
            acq->set_doppler_step(static_cast<unsigned int>(config.property(role + ".doppler_step", 250)));
            acq->set_threshold(threshold);
            acq->init();
            acq->set_local_code();
        }
    catch (const std::exception& e)
        {
            return report_error("configured", e);
        }

    const size_t N = block->fft_size();
    gsdr_stream* ring = nullptr;
    if (use_ring)
        {
            if (gsdr_stream_create(0, GSDR_ITEM_GR_COMPLEX, x.size(), static_cast<uint64_t>(block->batch_items()) * N, &ring) !=
                    GSDR_OK ||
                gsdr_stream_push(ring, x.data(), 0, x.size()) != GSDR_OK)
                {
                    std::cerr << "ring: " << gsdr_last_error() << '\n';
                    return 1;
                }
            block->set_ring(ring, 0);
        }

    std::printf("{\"built\": true, \"implementation\": \"%s\", \"item_size\": %zu, \"item_samples\": %zu, "
                "\"vector_length\": %u, \"code_length\": %u, \"num_doppler_bins\": %u, \"doppler_max\": %u, "
                "\"sampled_ms\": %u, \"coherent_ms\": %u, \"max_dwells\": %u, \"caf_window_hz\": %d, "
                "\"zero_padding\": %d, \"bit_transition_flag\": %s, \"both_components\": %s, "
                "\"threshold\": %.9g, \"attempts\": [",
        acq->implementation().c_str(), acq->item_size(), N, adapter->vector_length(), adapter->code_length(),
        block->num_doppler_bins(), adapter->doppler_max(), adapter->sampled_ms(), block->coherent_ms(),
        adapter->max_dwells(), adapter->CAF_window_hz(), adapter->zero_padding(),
        adapter->bit_transition_flag() ? "true" : "false", block->both_signal_components() ? "true" : "false",
        adapter->threshold());
    size_t offset = 0;
    for (int a = 0; a < attempts; ++a)
        {
            acq->reset();
            event = 0;
            std::printf("%s{\"start\": %zu, \"calls\": [", a ? ", " : "", offset);
            bool first = true;
            while (event == 0 && offset + N <= x.size())
                {
                    const int offered = static_cast<int>(std::min<size_t>(per_call, (x.size() - offset) / N));
                    const int state = block->state();
                    Gnss_Synchro monitor;
                    int produced = 0;
                    const int c = block->work(x.data() + offset, offered, &monitor, &produced);
                    offset += static_cast<size_t>(c) * N;
                    std::printf("%s{\"state\": %d, \"offered\": %d, \"consumed\": %d, \"event\": %d, "
                                "\"acq_delay_samples\": %.17g, \"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, "
                                "\"acq_doppler_step\": %u, \"mag\": %.9g, \"input_power\": %.9g, \"well_count\": %u, "
                                "\"test_statistics\": %.9g, \"monitor\": ",
                        first ? "" : ", ", state, offered, c, event, synchro.Acq_delay_samples, synchro.Acq_doppler_hz,
                        static_cast<unsigned long long>(synchro.Acq_samplestamp_samples), synchro.Acq_doppler_step,
                        block->mag_value(), block->input_power(), block->well_count(), block->test_statistics());
                    if (produced)
                        std::printf("{\"acq_delay_samples\": %.17g, \"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, "
                                    "\"acq_doppler_step\": %u, \"prn\": %u}}",
                            monitor.Acq_delay_samples, monitor.Acq_doppler_hz,
                            static_cast<unsigned long long>(monitor.Acq_samplestamp_samples), monitor.Acq_doppler_step,
                            monitor.PRN);
                    else
                        std::printf("null}");
                    first = false;
                }
            std::printf("], \"event\": %d, \"end_state\": %d, \"sample_counter\": %llu}", event, block->state(),
                static_cast<unsigned long long>(block->sample_counter()));
        }
    std::printf("]}\n");
    acq.reset();
    if (ring) gsdr_stream_destroy(ring);
    return 0;
}
