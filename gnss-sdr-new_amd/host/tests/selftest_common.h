// What the .conf-driven self-test programs have in common: reading the .conf and the IQ file,
// building the role's block through the factory with its refusal reported as a JSON line, the
// channel's configure sequence, the device ring, and the attempts-and-calls loop of the item-wise
// acquisition blocks with the JSON fields every one of them prints.
#ifndef GSDR_HOST_TESTS_SELFTEST_COMMON_H
#define GSDR_HOST_TESTS_SELFTEST_COMMON_H

#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "acquisition_item_block_mi355x.h"
#include "configuration.h"
#include "gnss_block_factory_mi355x.h"
#include "gsdr.h"

namespace selftest
{
inline std::string trim(const std::string& s)
{
    const auto a = s.find_first_not_of(" \t\r\n");
    if (a == std::string::npos) return "";
    return s.substr(a, s.find_last_not_of(" \t\r\n") - a + 1);
}

// a GNSS-SDR style .conf: name=value lines, ';' comments, [sections] skipped
inline bool read_conf(const std::string& path, InMemoryConfiguration& config)
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

// the gr_complex samples of a file
inline bool read_iq(const std::string& path, std::vector<std::complex<float>>& x)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    x.resize(static_cast<size_t>(f.tellg()) / sizeof(std::complex<float>));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(x.data()), static_cast<std::streamsize>(x.size() * sizeof(std::complex<float>)));
    return true;
}

// argv[1] into config and argv[2] into x; says which one cannot be read
inline bool read_inputs(char** argv, InMemoryConfiguration& config, std::vector<std::complex<float>>& x)
{
    const bool conf_read = read_conf(argv[1], config);
    if (!conf_read || !read_iq(argv[2], x))
        {
            std::cerr << "cannot read " << argv[conf_read ? 2 : 1] << '\n';
            return false;
        }
    return true;
}

// the JSON line of a refusal at stage "built" or "configured"; returns the exit status
inline int report_error(const char* stage, const std::exception& e)
{
    std::string what = e.what();
    std::replace(what.begin(), what.end(), '"', '\'');
    std::cout << "{\"built\": " << (std::string(stage) == "built" ? "false" : "true, \"configured\": false")
              << ", \"error\": \"" << what << "\"}\n";
    return 1;
}

// the role's acquisition block from the factory; null, with the JSON line printed, where it refuses
inline std::unique_ptr<AcquisitionInterface> build_acquisition(const InMemoryConfiguration& config, const std::string& role)
{
    std::unique_ptr<AcquisitionInterface> acq;
    try
        {
            acq = gsdr_factory::GetAcqBlock(&config, role, 1, 0, 0);
        }
    catch (const std::exception& e)
        {
            report_error("built", e);
            return nullptr;
        }
    if (!acq) std::cout << "{\"built\": false}\n";
    return acq;
}

// the block as the adapter the program drives; null, with the JSON line printed, for any other
template <class Adapter>
Adapter* expect_adapter(AcquisitionInterface* acq, const char* key)
{
    auto* adapter = dynamic_cast<Adapter*>(acq);
    if (!adapter)
        std::cout << "{\"built\": true, \"implementation\": \"" << acq->implementation() << "\", \"" << key << "\": false}\n";
    return adapter;
}

// the Doppler grid before the threshold: the adapter's pfa threshold counts its rows
inline void configure(AcquisitionInterface* acq, const InMemoryConfiguration& config, const std::string& role,
    Gnss_Synchro* synchro, float threshold)
{
    acq->set_channel(0);
    acq->set_gnss_synchro(synchro);
    acq->set_doppler_max(static_cast<unsigned int>(config.property(role + ".doppler_max", 5000)));
    acq->set_doppler_step(static_cast<unsigned int>(config.property(role + ".doppler_step", 250)));
    acq->set_threshold(threshold);
    acq->init();
    acq->set_local_code();
}

// configure(), a refusal reported as the JSON line of stage "configured"
inline bool configure_or_report(AcquisitionInterface* acq, const InMemoryConfiguration& config, const std::string& role,
    Gnss_Synchro* synchro, float threshold)
{
    try
        {
            configure(acq, config, role, synchro, threshold);
        }
    catch (const std::exception& e)
        {
            report_error("configured", e);
            return false;
        }
    return true;
}

// a device ring of all of x with a reader window of `window` samples; null, with a message, on failure
inline gsdr_stream* make_ring(const std::vector<std::complex<float>>& x, uint64_t window)
{
    gsdr_stream* ring = nullptr;
    if (gsdr_stream_create(0, GSDR_ITEM_GR_COMPLEX, x.size(), window, &ring) != GSDR_OK ||
        gsdr_stream_push(ring, x.data(), 0, x.size()) != GSDR_OK)
        {
            std::cerr << "ring: " << gsdr_last_error() << '\n';
            return nullptr;
        }
    return ring;
}

// "monitor": the Gnss_Synchro a call produced, or null; closes the call's object
inline void print_monitor(const Gnss_Synchro* monitor)
{
    if (monitor)
        std::printf("\"monitor\": {\"acq_delay_samples\": %.17g, \"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, "
                    "\"acq_doppler_step\": %u, \"prn\": %u}}",
            monitor->Acq_delay_samples, monitor->Acq_doppler_hz,
            static_cast<unsigned long long>(monitor->Acq_samplestamp_samples), monitor->Acq_doppler_step, monitor->PRN);
    else
        std::printf("\"monitor\": null}");
}

// `attempts` acquisitions one after the other over the items of N samples in x (reset() after each
// event, which the block's handler writes to `event`), per_call items offered to every call.
// Prints the "attempts" array and closes the JSON line.  work(in, offered, &monitor, &produced)
// is the block's work(); print_fields(monitor) prints the block's own fields of one call after the
// shared ones and closes the call's object (monitor: what the call produced, or null).
template <class Work, class PrintFields>
void run_attempts(AcquisitionInterface* acq, const acquisition_item_block_mi355x* block, const Gnss_Synchro& synchro,
    int& event, const std::vector<std::complex<float>>& x, size_t N, int attempts, int per_call, Work work,
    PrintFields print_fields)
{
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
                    const int c = work(x.data() + offset, offered, &monitor, &produced);
                    offset += static_cast<size_t>(c) * N;
                    std::printf("%s{\"state\": %d, \"offered\": %d, \"consumed\": %d, \"event\": %d, "
                                "\"acq_delay_samples\": %.17g, \"acq_doppler_hz\": %.17g, \"acq_samplestamp_samples\": %llu, "
                                "\"acq_doppler_step\": %u, \"mag\": %.9g, \"input_power\": %.9g, ",
                        first ? "" : ", ", state, offered, c, event, synchro.Acq_delay_samples, synchro.Acq_doppler_hz,
                        static_cast<unsigned long long>(synchro.Acq_samplestamp_samples), synchro.Acq_doppler_step,
                        block->mag_value(), block->input_power());
                    print_fields(produced ? &monitor : nullptr);
                    first = false;
                }
            std::printf("], \"event\": %d, \"end_state\": %d, \"sample_counter\": %llu}", event, block->state(),
                static_cast<unsigned long long>(block->sample_counter()));
        }
    std::printf("]}\n");
}
}  // namespace selftest

#endif
