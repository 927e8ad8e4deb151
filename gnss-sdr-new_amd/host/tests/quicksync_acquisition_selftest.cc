// Self-test driver of the GPS L1 C/A QuickSync acquisition block (tests/test_host_quicksync.py).
//
//   quicksync_acquisition_selftest <file.conf> <iq.dat> <prn> <threshold> <attempts> <ring 0|1> [items per call]
//
// Reads a GNSS-SDR style .conf (name=value lines, ';' comments), builds the Acquisition_1C
// block from it through the block factory, and feeds it the gr_complex samples of iq.dat as
// items of folding_factor code periods through its state machine, `attempts` acquisitions one after the
// other (reset() after each event), offering `items per call` items (default 1) to every
// work() call.  With ring = 1 the samples are also pushed into a device ring and the block
// reads its items there.  Prints one JSON line: per attempt, for every work() call the state
// before it, the items it consumed, the event it published (0: none) and the Gnss_Synchro
// acquisition fields after it.
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
#include "gps_l1_ca_pcps_quicksync_acquisition_mi355x.h"
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
}  // namespace

int main(int argc, char** argv)
{
    if (argc < 7)
        {
            std::cerr << "usage: quicksync_acquisition_selftest <file.conf> <iq.dat> <prn> <threshold> <attempts> <ring> "
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
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[3]));
    const float threshold = static_cast<float>(std::atof(argv[4]));
    const int attempts = std::atoi(argv[5]);
    const bool use_ring = std::atoi(argv[6]) != 0;
    const int per_call = argc > 7 ? std::max(1, std::atoi(argv[7])) : 1;

    const std::string role = "Acquisition_1C";
    std::unique_ptr<AcquisitionInterface> acq;
    try
        {
            acq = gsdr_factory::GetAcqBlock(&config, role, 1, 0, 0);
        }
    catch (const std::exception& e)
        {
            std::string what = e.what();
            std::replace(what.begin(), what.end(), '"', '\'');
            std::cout << "{\"built\": false, \"error\": \"" << what << "\"}\n";
            return 1;
        }
    if (!acq)
        {
            std::cout << "{\"built\": false}\n";
            return 1;
        }
    auto* adapter = dynamic_cast<GpsL1CaPcpsQuickSyncAcquisitionMI355X*>(acq.get());
    if (!adapter)
        {
            std::cout << "{\"built\": true, \"implementation\": \"" << acq->implementation() << "\", \"quicksync\": false}\n";
            return 1;
        }
    pcps_quicksync_acquisition_mi355x* block = adapter->get_block();
    Gnss_Synchro synchro;
    synchro.System = 'G';
    synchro.Signal[0] = '1';
    synchro.Signal[1] = 'C';
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
            std::string what = e.what();
            std::replace(what.begin(), what.end(), '"', '\'');
            std::cout << "{\"built\": true, \"configured\": false, \"error\": \"" << what << "\"}\n";
            return 1;
        }

    const size_t N = block->item_samples();
    gsdr_stream* ring = nullptr;
    if (use_ring)
        {
            if (gsdr_stream_create(0, GSDR_ITEM_GR_COMPLEX, x.size(), N, &ring) != GSDR_OK ||
                gsdr_stream_push(ring, x.data(), 0, x.size()) != GSDR_OK)
                {
                    std::cerr << "ring: " << gsdr_last_error() << '\n';
                    return 1;
                }
            block->set_ring(ring, 0);
        }

    std::printf("{\"built\": true, \"implementation\": \"%s\", \"item_size\": %zu, \"item_samples\": %zu, "
                "\"fft_size\": %u, \"folding_factor\": %u, \"num_doppler_bins\": %u, \"max_dwells\": %u, "
                "\"doppler_max\": %u, \"sampled_ms\": %u, \"bit_transition_flag\": %d, \"threshold\": %.9g, "
                "\"attempts\": [",
        acq->implementation().c_str(), acq->item_size(), N, block->fft_size(), adapter->folding_factor(),
        block->num_doppler_bins(), adapter->max_dwells(), adapter->doppler_max(), adapter->sampled_ms(),
        adapter->bit_transition_flag() ? 1 : 0, adapter->threshold());
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
                    const int c = block->work(x.data() + offset, offered);
                    offset += static_cast<size_t>(c) * N;
                    std::printf("%s{\"state\": %d, \"offered\": %d, \"consumed\": %d, \"event\": %d, "
                                "\"acq_delay_samples\": %.17g, \"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, "
                                "\"acq_doppler_step\": %u, \"mag\": %.9g, \"input_power\": %.9g, \"test_statistic\": %.9g}",
                        first ? "" : ", ", state, offered, c, event, synchro.Acq_delay_samples, synchro.Acq_doppler_hz,
                        static_cast<unsigned long long>(synchro.Acq_samplestamp_samples), synchro.Acq_doppler_step,
                        block->mag_value(), block->input_power(), block->test_statistics());
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
