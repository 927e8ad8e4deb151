// Self-test driver of the GPS L1 C/A Kalman tracking adapter (tests/test_gpu_trk_kf.py).
//
//   kf_tracking_selftest <file.conf> <iq.dat> <role> <prn> <acq delay samples> <acq doppler hz>
//
// Reads a GNSS-SDR style .conf (name=value lines, ';' comments), builds the block of <role>
// (Tracking_1C, implementation GPS_L1_CA_KF_Tracking_MI355X) from it through the block factory, starts it as the channel would after an acquisition at
// stamp 0 and feeds it the gr_complex samples of iq.dat through work() in scheduler-sized
// chunks (per-channel or pooled block, as <role>.mi355x_pool says).  Prints one JSON line:
// whether the block was built (with the refusal's text if not), and for every Gnss_Synchro
// it emitted the sample counter, Prompt_I, Prompt_Q, correlation_length_ms and the flags;
// beside them, per engine record that carried a valid output, the record's own prompt pair.
#include <algorithm>
#include <cstdlib>

#include "gnss_tracking_mi355x.h"
#include "selftest_common.h"

int main(int argc, char** argv)
{
    if (argc < 7)
        {
            std::cerr << "usage: kf_tracking_selftest <file.conf> <iq.dat> <role> <prn> <acq delay samples> <acq doppler hz>\n";
            return 2;
        }
    InMemoryConfiguration config;
    std::vector<std::complex<float>> x;
    if (!selftest::read_inputs(argv, config, x)) return 2;
    const std::string role = argv[3];

    std::unique_ptr<TrackingInterface> trk;
    try
        {
            trk = gsdr_factory::GetTrkBlock(&config, role, 1, 1, 0);
        }
    catch (const std::exception& e)
        {
            return selftest::report_error("built", e);
        }
    auto* adapter = dynamic_cast<GpsL1CaKfTrackingMI355X*>(trk.get());
    if (!adapter)
        {
            std::cout << "{\"built\": false, \"error\": \"not the GPS L1 C/A Kalman tracking adapter\"}\n";
            return 1;
        }
    Gnss_Synchro gs;
    gs.System = 'G';
    gs.Signal[0] = '1';
    gs.Signal[1] = 'C';
    gs.PRN = static_cast<uint32_t>(std::atoi(argv[4]));
    gs.Acq_delay_samples = std::atof(argv[5]);
    gs.Acq_doppler_hz = std::atof(argv[6]);
    gs.Acq_samplestamp_samples = 0;
    trk->set_channel(0);
    trk->set_gnss_synchro(&gs);
    trk->start_tracking();
    auto* blk = adapter->get_block();
    std::vector<gsdr_trk_epoch> valid;
    blk->set_record_sink([&valid](const gsdr_trk_epoch& e) {
        if (e.flags & GSDR_TRK_F_VALID_OUTPUT) valid.push_back(e);
    });
    std::vector<Gnss_Synchro> outs;
    uint64_t nread = 0;
    for (;;)
        {
            if (nread + static_cast<uint64_t>(blk->forecast()) > x.size()) break;
            const int avail = static_cast<int>(std::min<uint64_t>(16384, x.size() - nread));
            Gnss_Synchro out{};
            int nout = 0;
            const int used = blk->work(x.data() + nread, avail, nread, &out, &nout);
            if (nout == 1) outs.push_back(out);
            if (used <= 0 && nout == 0) break;
            nread += static_cast<uint64_t>(std::max(used, 0));
        }
    blk->flush();
    for (int guard = 0; guard < 100000; ++guard)
        {
            Gnss_Synchro out{};
            int nout = 0;
            blk->work(nullptr, 0, nread, &out, &nout);
            if (nout == 0) break;
            outs.push_back(out);
        }
    std::printf("{\"built\": true, \"pooled\": %s, \"vector_length\": %u, \"kf\": %s, \"extend\": %d, \"track_pilot\": %s, "
                "\"bit_sync_limit_s\": %u, \"outputs\": [",
        adapter->pooled() ? "true" : "false", adapter->conf().vector_length, adapter->conf().kf ? "true" : "false",
        adapter->conf().extend_correlation_symbols, adapter->conf().track_pilot ? "true" : "false",
        adapter->conf().bit_synchronization_time_limit_s);
    for (size_t i = 0; i < outs.size(); ++i)
        std::printf("%s[%llu, %.17g, %.17g, %d, %d, %d]", i ? ", " : "", static_cast<unsigned long long>(outs[i].Tracking_sample_counter),
            outs[i].Prompt_I, outs[i].Prompt_Q, outs[i].correlation_length_ms, outs[i].Flag_valid_symbol_output ? 1 : 0,
            outs[i].Flag_PLL_180_deg_phase_locked ? 1 : 0);
    std::printf("], \"records\": [");
    for (size_t i = 0; i < valid.size(); ++i)
        std::printf("%s[%llu, %.17g, %.17g, %.9g, %.9g]", i ? ", " : "", static_cast<unsigned long long>(valid[i].sample_counter),
            valid[i].prompt_i, valid[i].prompt_q, valid[i].data_prompt[0], valid[i].data_prompt[1]);
    std::printf("]}\n");
    return 0;
}
