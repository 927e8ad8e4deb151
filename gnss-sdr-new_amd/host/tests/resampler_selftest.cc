// GNSS-SDR.use_acquisition_resampler on the device ring path (acq_resampler.h,
// AcquisitionService::attach_resampler, gsdr_factory::GetAcqService), on the GPU:
//   1. the hub hands two services of one (device, ring key, signal) the same
//      decimator, another signal its own, and none without the switch;
//   2. synthetic GPS L1 C/A at 16 Msps through a service with the resampler attached
//      (decimation 8, 39 taps, PCPS at 2 Msps): the strong satellite is answered
//      positive, its delay -- mapped back to the input rate as
//      pcps_acquisition.cc:699-705 does -- within one decimated sample of the truth,
//      its Doppler within one step, its stamp a multiple of the input-rate block.
// Prints "resampler_selftest: PASS" and exits 0 when every check holds.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "acq_resampler.h"
#include "acquisition_service.h"
#include "configuration.h"
#include "gnss_block_factory_mi355x.h"
#include "gnss_replicas.h"
#include "gsdr.h"
#include "synth_stream.h"

namespace
{
int failures = 0;

#define EXPECT(cond, msg)                                              \
    do                                                                 \
        {                                                              \
            if (!(cond))                                               \
                {                                                      \
                    std::cerr << "FAIL: " << msg << " (" #cond ")\n"; \
                    ++failures;                                        \
                }                                                      \
        }                                                              \
    while (0)

constexpr double kFs = 16000000.0;
constexpr uint32_t kDecimation = 8;     // floor(16 / 2)
constexpr uint32_t kLatency = 19;       // (39 taps - 1) / 2
constexpr uint64_t kBlockIn = 16000;    // 1 ms at the input rate

InMemoryConfiguration config_16msps(bool resampler, const std::string& item_type)
{
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "16000000");
    config.set_property("GNSS-SDR.use_acquisition_resampler", resampler ? "true" : "false");
    for (const char* role : {"Acquisition_1C", "Acquisition_1B"})
        {
            config.set_property(std::string(role) + ".item_type", item_type);
            config.set_property(std::string(role) + ".pfa", "0.01");
            config.set_property(std::string(role) + ".doppler_max", "5000");
            config.set_property(std::string(role) + ".doppler_step", "250");
        }
    config.set_property("Acquisition_1C.coherent_integration_time_ms", "1");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "4");
    return config;
}

void test_hub_shares_one_decimator()
{
    gsdr_stream* ring = nullptr;
    EXPECT(gsdr_stream_create(0, GSDR_ITEM_GR_COMPLEX, 64 * kBlockIn, 32 * kBlockIn, &ring) == GSDR_OK, "source ring");
    if (!ring) return;
    {
        InMemoryConfiguration on = config_16msps(true, "gr_complex"), off = config_16msps(false, "gr_complex");
        auto a = gsdr_factory::GetAcqService(&on, "Acquisition_1C", "1C", 4, ring, "hub_test");
        auto b = gsdr_factory::GetAcqService(&on, "Acquisition_1C", "1C", 2, ring, "hub_test");
        auto e = gsdr_factory::GetAcqService(&on, "Acquisition_1B", "1B", 2, ring, "hub_test");
        auto o = gsdr_factory::GetAcqService(&on, "Acquisition_1C", "1C", 2, ring, "another_stream");
        auto n = gsdr_factory::GetAcqService(&off, "Acquisition_1C", "1C", 2, ring, "hub_test");
        EXPECT(a && b && e && o && n, "factory builds the services");
        if (a && b && e && o && n)
            {
                EXPECT(a->resampler() && a->resampler() == b->resampler(), "one key, one decimator");
                EXPECT(a->resampler()->output() == b->resampler()->output(), "one key, one decimated ring");
                EXPECT(e->resampler() && e->resampler() != a->resampler(), "another signal, another decimator");
                EXPECT(o->resampler() && o->resampler() != a->resampler(), "another stream key, another decimator");
                EXPECT(!n->resampler(), "no switch, no resampler");
                EXPECT(a->resampler()->decimation() == kDecimation && a->resampler()->taps().size() == 39 &&
                           a->resampler()->latency() == kLatency,
                    "16 Msps GPS: decimation 8, 39 taps, latency 19");
                EXPECT(a->conf().resampled_fs == 2000000 && n->conf().resampled_fs == 16000000, "Acq_Conf rates");
                uint32_t d = 0, t = 0, lat = 0;
                EXPECT(gsdr_acq_resampler_plan(16000000, 2000000.0, &d, &t, &lat) == GSDR_OK && d == kDecimation && t == 39 &&
                           lat == kLatency,
                    "gsdr_acq_resampler_plan agrees with the hub");
                // a service whose configuration asks for no resampler takes none
                n->work_ring(ring, 0);
                bool threw = false;
                try
                    {
                        n->attach_resampler(a->resampler());
                    }
                catch (const std::exception&)
                    {
                        threw = true;
                    }
                EXPECT(threw, "attach_resampler on a service without the switch throws");
            }
    }  // the services (and the decimators they held) before their source
    gsdr_stream_destroy(ring);
}

void test_service_on_decimated_ring(const std::string& item_type)
{
    const double sigma = 1.0;
    const double amp = std::sqrt(2.0 * std::pow(10.0, 5.0) / kFs) * sigma;  // 50 dB-Hz
    // The truth: the code starts at input sample `delay`.  PCPS reports where the
    // reference's sampled replica lines up, and that replica puts sample i at code time
    // (i + 1) / fs (gps_l1_ca_code_gen_complex_sampled: ceil((i + 1) ts / tc) - 1), so
    // on the decimated ring the peak sits at round(k0 + 1), k0 = (delay + latency) / d:
    // one decimated sample after the code start, plus the rounding to the 2 Msps grid.
    // (The full-rate tests absorb the same sample in their half-chip tolerances; an fp64
    // model of filter, decimation and correlation gives the same peak.)  The bound below
    // is one decimated sample, so the delay is chosen with frac(k0) = 0.25: the rounding
    // then goes towards the truth and the expected error is 0.75 d = 6 input samples.
    const double delay = 5239.0, doppler = 1680.0;
    SynthSat sat{gps_l1_ca_code_gen_float(1), 1.023e6, 1575.42e6, delay, doppler, amp, {}, {}, 0.02};
    const auto x = synth_stream({sat}, kFs, static_cast<size_t>(kFs * 0.020), 23, sigma);
    const bool cshort = item_type == "cshort";
    std::vector<int16_t> xs;
    if (cshort)
        {
            xs.resize(2 * x.size());
            for (size_t i = 0; i < x.size(); ++i)
                {
                    xs[2 * i] = static_cast<int16_t>(std::lrint(x[i].real() * 1000.0F));
                    xs[2 * i + 1] = static_cast<int16_t>(std::lrint(x[i].imag() * 1000.0F));
                }
        }
    gsdr_stream* ring = nullptr;
    EXPECT(gsdr_stream_create(0, cshort ? GSDR_ITEM_CSHORT : GSDR_ITEM_GR_COMPLEX, 64 * kBlockIn, 32 * kBlockIn, &ring) ==
               GSDR_OK,
        "source ring");
    if (!ring) return;
    {
        InMemoryConfiguration config = config_16msps(true, item_type);
        auto svc = gsdr_factory::GetAcqService(&config, "Acquisition_1C", "1C", 2, ring, "svc_" + item_type);
        EXPECT(svc && svc->resampler(), "service with the resampler attached");
        if (svc && svc->resampler())
            {
                // the replicas at the rate the grid runs at
                const auto fs_acq = static_cast<int32_t>(svc->conf().resampled_fs);
                const auto code1 = gps_l1_ca_code_gen_complex_sampled(1, fs_acq, 0);
                const auto code9 = gps_l1_ca_code_gen_complex_sampled(9, fs_acq, 0);
                EXPECT(fs_acq == 2000000 && code1.size() == 2000, "replica at 2 Msps");
                gsdr_acq_result got[2]{};
                bool pos[2] = {false, false};
                int answered[2] = {0, 0};
                auto cb = [&](uint32_t c, const gsdr_acq_result& r, bool p) {
                    got[c] = r;
                    pos[c] = p;
                    ++answered[c];
                };
                svc->request(0, 1, code1.data(), cb);
                svc->request(1, 9, code9.data(), cb);
                svc->work_ring(ring, 0);  // origin of the block grid
                size_t at = 0;
                bool pushed_all = true;
                while (at < x.size())
                    {
                        const size_t n = std::min<size_t>(4096, x.size() - at);
                        const void* src = cshort ? static_cast<const void*>(xs.data() + 2 * at)
                                                 : static_cast<const void*>(x.data() + at);
                        if (gsdr_stream_push(ring, src, at, n) != GSDR_OK)
                            {
                                pushed_all = false;
                                break;
                            }
                        at += n;
                        svc->work_ring(ring, at);  // the SOURCE ring and head
                    }
                svc->flush();
                EXPECT(pushed_all, "pushes");
                EXPECT(answered[0] == 1 && answered[1] == 1, "both requests answered once");
                EXPECT(pos[0], "PRN 1 (50 dB-Hz) positive on the decimated ring");
                EXPECT(!pos[1], "PRN 9 (absent) negative");
                // delay at the input rate, within one decimated sample (code period 16000 input samples)
                double err = std::fmod(got[0].acq_delay_samples - delay, static_cast<double>(kBlockIn));
                if (err > kBlockIn / 2.0) err -= static_cast<double>(kBlockIn);
                if (err < -(kBlockIn / 2.0)) err += static_cast<double>(kBlockIn);
                EXPECT(std::abs(err) <= static_cast<double>(kDecimation), "delay within one decimated sample of the truth");
                // what the mapping did: code_phase is the decimated-rate index
                EXPECT(got[0].acq_delay_samples ==
                           static_cast<double>(got[0].code_phase) * kDecimation - static_cast<double>(kLatency),
                    "acq_delay_samples = code phase x ratio - latency");
                EXPECT(std::abs(static_cast<double>(got[0].doppler_hz) - doppler) <= 250.0, "Doppler within one step");
                EXPECT(got[0].samplestamp > 0 && got[0].samplestamp % kBlockIn == 0 && got[0].samplestamp <= x.size(),
                    "stamp: a multiple of the block length at the input rate");
                EXPECT(svc->grids_run() >= 4, "batches ran");
                std::printf("resampled service (%s): PRN1 positive %d delay %.1f (truth %.1f) doppler %d Hz stamp %llu; "
                            "PRN9 positive %d; %llu blocks\n",
                    item_type.c_str(), pos[0] ? 1 : 0, got[0].acq_delay_samples, delay, got[0].doppler_hz,
                    static_cast<unsigned long long>(got[0].samplestamp), pos[1] ? 1 : 0,
                    static_cast<unsigned long long>(svc->grids_run()));
            }
    }
    gsdr_stream_destroy(ring);
}
}  // namespace

int main()
{
    int ndev = 0;
    if (gsdr_device_count(&ndev) != GSDR_OK || ndev < 1)
        {
            std::cerr << "resampler_selftest: no HIP device\n";
            return 2;
        }
    try
        {
            test_hub_shares_one_decimator();
            test_service_on_decimated_ring("gr_complex");
            test_service_on_decimated_ring("cshort");
        }
    catch (const std::exception& e)
        {
            std::cerr << "FAIL: exception: " << e.what() << '\n';
            ++failures;
        }
    if (failures)
        {
            std::cerr << "resampler_selftest: " << failures << " check(s) failed\n";
            return 1;
        }
    std::printf("resampler_selftest: PASS\n");
    return 0;
}
