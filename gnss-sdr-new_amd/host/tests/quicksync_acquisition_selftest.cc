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
#include <cstdlib>

#include "gps_l1_ca_pcps_quicksync_acquisition_mi355x.h"
#include "selftest_common.h"

int main(int argc, char** argv)
{
    if (argc < 7)
        {
            std::cerr << "usage: quicksync_acquisition_selftest <file.conf> <iq.dat> <prn> <threshold> <attempts> <ring> "
                         "[items per call]\n";
            return 2;
        }
    InMemoryConfiguration config;
    std::vector<std::complex<float>> x;
    if (!selftest::read_inputs(argv, config, x)) return 2;
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[3]));
    const float threshold = static_cast<float>(std::atof(argv[4]));
    const int attempts = std::atoi(argv[5]);
    const bool use_ring = std::atoi(argv[6]) != 0;
    const int per_call = argc > 7 ? std::max(1, std::atoi(argv[7])) : 1;

    const std::string role = "Acquisition_1C";
    auto acq = selftest::build_acquisition(config, role);
    if (!acq) return 1;
    auto* adapter = selftest::expect_adapter<GpsL1CaPcpsQuickSyncAcquisitionMI355X>(acq.get(), "quicksync");
    if (!adapter) return 1;
    pcps_quicksync_acquisition_mi355x* block = adapter->get_block();
    Gnss_Synchro synchro;
    synchro.System = 'G';
    synchro.Signal[0] = '1';
    synchro.Signal[1] = 'C';
    synchro.PRN = prn;
    int event = 0;
    block->set_event_handler([&event](int e) { event = e; });
    if (!selftest::configure_or_report(acq.get(), config, role, &synchro, threshold)) return 1;

    const size_t N = block->item_samples();
    gsdr_stream* ring = nullptr;
    if (use_ring)
        {
            ring = selftest::make_ring(x, N);
            if (!ring) return 1;
            block->set_ring(ring, 0);
        }

    std::printf("{\"built\": true, \"implementation\": \"%s\", \"item_size\": %zu, \"item_samples\": %zu, "
                "\"fft_size\": %u, \"folding_factor\": %u, \"num_doppler_bins\": %u, \"max_dwells\": %u, "
                "\"doppler_max\": %u, \"sampled_ms\": %u, \"bit_transition_flag\": %d, \"threshold\": %.9g, "
                "\"attempts\": [",
        acq->implementation().c_str(), acq->item_size(), N, block->fft_size(), adapter->folding_factor(),
        block->num_doppler_bins(), adapter->max_dwells(), adapter->doppler_max(), adapter->sampled_ms(),
        adapter->bit_transition_flag() ? 1 : 0, adapter->threshold());
    selftest::run_attempts(
        acq.get(), block, synchro, event, x, N, attempts, per_call,
        [block](const std::complex<float>* in, int offered, Gnss_Synchro*, int*) { return block->work(in, offered); },
        [block](const Gnss_Synchro*) { std::printf("\"test_statistic\": %.9g}", block->test_statistics()); });
    acq.reset();
    if (ring) gsdr_stream_destroy(ring);
    return 0;
}
