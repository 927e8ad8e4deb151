// Self-test driver of the two Tong acquisition blocks (tests/test_host_tong.py).
//
//   tong_acquisition_selftest <file.conf> <iq.dat> <role> <prn> <threshold> <attempts> <ring 0|1> [items per call]
//
// Reads a GNSS-SDR style .conf (name=value lines, ';' comments), builds the block of <role>
// (Acquisition_1C or Acquisition_1B) from it through the block factory, and feeds it the
// gr_complex samples of iq.dat as items of the adapter's vector length through its state
// machine, `attempts` acquisitions one after the other (reset() after each event), offering
// `items per call` items (default 1) to every work() call.  With ring = 1 the samples are also
// pushed into a device ring and the block reads its items there.  Prints one JSON line: per
// attempt, for every work() call the state before it, the items it consumed, the event it
// published (0: none), the counters, the Gnss_Synchro acquisition fields after it and the
// monitor output, if the call produced one.
#include <algorithm>
#include <cstdlib>

#include "gps_l1_ca_pcps_tong_acquisition_mi355x.h"
#include "selftest_common.h"

int main(int argc, char** argv)
{
    if (argc < 8)
        {
            std::cerr << "usage: tong_acquisition_selftest <file.conf> <iq.dat> <role> <prn> <threshold> <attempts> <ring> "
                         "[items per call]\n";
            return 2;
        }
    InMemoryConfiguration config;
    std::vector<std::complex<float>> x;
    if (!selftest::read_inputs(argv, config, x)) return 2;
    const std::string role = argv[3];
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[4]));
    const float threshold = static_cast<float>(std::atof(argv[5]));
    const int attempts = std::atoi(argv[6]);
    const bool use_ring = std::atoi(argv[7]) != 0;
    const int per_call = argc > 8 ? std::max(1, std::atoi(argv[8])) : 1;

    auto acq = selftest::build_acquisition(config, role);
    if (!acq) return 1;
    auto* adapter = selftest::expect_adapter<PcpsTongAcquisitionAdapterMI355X>(acq.get(), "tong");
    if (!adapter) return 1;
    pcps_tong_acquisition_mi355x* block = adapter->get_block();
    Gnss_Synchro synchro;
    const bool galileo = role == "Acquisition_1B";
    synchro.System = galileo ? 'E' : 'G';
    synchro.Signal[0] = '1';
    synchro.Signal[1] = galileo ? 'B' : 'C';
    synchro.PRN = prn;
    int event = 0;
    block->set_event_handler([&event](int e) { event = e; });
    if (!selftest::configure_or_report(acq.get(), config, role, &synchro, threshold)) return 1;

    const size_t N = block->fft_size();
    gsdr_stream* ring = nullptr;
    if (use_ring)
        {
            ring = selftest::make_ring(x, static_cast<uint64_t>(block->batch_items()) * N);
            if (!ring) return 1;
            block->set_ring(ring, 0);
        }

    std::printf("{\"built\": true, \"implementation\": \"%s\", \"item_size\": %zu, \"item_samples\": %zu, "
                "\"vector_length\": %u, \"code_length\": %u, \"num_doppler_bins\": %u, \"doppler_max\": %u, "
                "\"sampled_ms\": %u, \"tong_init_val\": %u, \"tong_max_val\": %u, \"tong_max_dwells\": %u, "
                "\"threshold\": %.9g, \"attempts\": [",
        acq->implementation().c_str(), acq->item_size(), N, adapter->vector_length(), adapter->code_length(),
        block->num_doppler_bins(), adapter->doppler_max(), adapter->sampled_ms(), adapter->tong_init_val(),
        adapter->tong_max_val(), adapter->tong_max_dwells(), adapter->threshold());
    selftest::run_attempts(
        acq.get(), block, synchro, event, x, N, attempts, per_call,
        [block](const std::complex<float>* in, int offered, Gnss_Synchro* monitor, int* produced) {
            return block->work(in, offered, monitor, produced);
        },
        [block](const Gnss_Synchro* monitor) {
            std::printf("\"dwell_count\": %u, \"tong_count\": %u, ", block->dwell_count(), block->tong_count());
            selftest::print_monitor(monitor);
        });
    acq.reset();
    if (ring) gsdr_stream_destroy(ring);
    return 0;
}
