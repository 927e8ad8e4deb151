// Self-test driver of the fine-Doppler acquisition block (tests/test_host_fine_doppler.py).
//
//   fine_doppler_selftest <file.conf> <iq.dat> <prn> <threshold> <attempts> <ring 0|1>
//
// Reads a GNSS-SDR style .conf (name=value lines, ';' comments), builds the Acquisition_1C
// block from it through the block factory, and feeds it the gr_complex samples of iq.dat as
// 1 ms items through its state machine, `attempts` acquisitions one after the other (reset()
// after each event).  With ring = 1 the samples are also pushed into a device ring and the
// block reads its 10 ms window there.  Prints one JSON line: per attempt the state before
// every work() call, the items each call consumed, the event, and the Gnss_Synchro
// acquisition fields afterwards.
#include <cstdlib>

#include "gps_l1_ca_pcps_acquisition_fine_doppler_mi355x.h"
#include "selftest_common.h"

int main(int argc, char** argv)
{
    if (argc < 7)
        {
            std::cerr << "usage: fine_doppler_selftest <file.conf> <iq.dat> <prn> <threshold> <attempts> <ring>\n";
            return 2;
        }
    InMemoryConfiguration config;
    std::vector<std::complex<float>> x;
    if (!selftest::read_inputs(argv, config, x)) return 2;
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[3]));
    const float threshold = static_cast<float>(std::atof(argv[4]));
    const int attempts = std::atoi(argv[5]);
    const bool use_ring = std::atoi(argv[6]) != 0;

    const std::string role = "Acquisition_1C";
    auto acq = gsdr_factory::GetAcqBlock(&config, role, 1, 0, 0);
    if (!acq)
        {
            std::cout << "{\"built\": false}\n";
            return 1;
        }
    auto* adapter = selftest::expect_adapter<GpsL1CaPcpsAcquisitionFineDopplerMI355X>(acq.get(), "fine");
    if (!adapter) return 1;
    pcps_acquisition_fine_doppler_mi355x* block = adapter->get_block();
    Gnss_Synchro synchro;
    synchro.System = 'G';
    synchro.Signal[0] = '1';
    synchro.Signal[1] = 'C';
    synchro.PRN = prn;
    int event = 0;
    block->set_event_handler([&event](int e) { event = e; });
    // the channel's set-up order (channel.cc: set_channel, set_gnss_synchro, threshold,
    // doppler_max, doppler_step, init, set_local_code)
    acq->set_channel(0);
    acq->set_gnss_synchro(&synchro);
    acq->set_threshold(threshold);
    acq->set_doppler_max(static_cast<unsigned int>(config.property(role + ".doppler_max", 5000)));
    acq->set_doppler_step(static_cast<unsigned int>(config.property(role + ".doppler_step", 500)));
    acq->init();
    acq->set_local_code();
    block->start();

    const int N = block->fft_size();
    gsdr_stream* ring = nullptr;
    if (use_ring)
        {
            ring = selftest::make_ring(x, 10ull * N);
            if (!ring) return 1;
            block->set_ring(ring, 0);
        }

    std::printf("{\"built\": true, \"implementation\": \"%s\", \"item_size\": %zu, \"fft_size\": %d, "
                "\"num_doppler_points\": %d, \"max_dwells\": %u, \"doppler_max\": %d, \"attempts\": [",
        acq->implementation().c_str(), acq->item_size(), N, block->num_doppler_points(), adapter->max_dwells(),
        adapter->doppler_max());
    size_t offset = 0;
    for (int a = 0; a < attempts; ++a)
        {
            acq->reset();
            event = 0;
            std::string states, consumed;
            const size_t start = offset;
            while (event == 0 && offset + static_cast<size_t>(N) <= x.size())
                {
                    states += (states.empty() ? "" : ", ") + std::to_string(block->state());
                    const int c = block->work(x.data() + offset, N);
                    consumed += (consumed.empty() ? "" : ", ") + std::to_string(c);
                    offset += static_cast<size_t>(c);
                }
            const gsdr_acq_fine_result& fr = block->last_fine_result();
            std::printf("%s{\"start\": %zu, \"states\": [%s], \"consumed\": [%s], \"event\": %d, \"end_state\": %d, "
                        "\"sample_counter\": %llu, \"test_statistic\": %.9g, \"mag\": %d, \"acq_delay_samples\": %.17g, "
                        "\"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, \"acq_doppler_step\": %u, "
                        "\"fine_index\": %u, \"fine_accepted\": %d, \"dump\": \"%s\"}",
                a ? ", " : "", start, states.c_str(), consumed.c_str(), event, block->state(),
                static_cast<unsigned long long>(block->sample_counter()), block->test_statistics(), acq->mag(),
                synchro.Acq_delay_samples, synchro.Acq_doppler_hz,
                static_cast<unsigned long long>(synchro.Acq_samplestamp_samples), synchro.Acq_doppler_step, fr.index,
                fr.accepted, block->last_dump_path().c_str());
        }
    std::printf("]}\n");
    acq.reset();
    if (ring) gsdr_stream_destroy(ring);
    return 0;
}
