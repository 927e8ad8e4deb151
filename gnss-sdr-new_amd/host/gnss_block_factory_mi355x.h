// Registration of the MI355X blocks: the GetAcqBlock / GetTrkBlock string
// switches of GNSSBlockFactory (src/core/receiver/gnss_block_factory.cc:1335-1519,
// :1522-1682) for the implementation names this engine provides, and the
// deterministic channel -> GPU map that replaces the CUDA path's per-instance
// rand() % num_devices (src/algorithms/tracking/libs/cuda_multicorrelator.cu:135-155).
//
// A maintainer adds the `if (implementation == "..._MI355X")` branches to the
// reference factory; here the same switch is a free function so
// the adapters can be built from a .conf without GNU Radio.
#ifndef GSDR_HOST_GNSS_BLOCK_FACTORY_MI355X_H
#define GSDR_HOST_GNSS_BLOCK_FACTORY_MI355X_H

#include <memory>
#include <string>

#include "acquisition_interface.h"
#include "acquisition_service.h"
#include "configuration.h"
#include "tracking_interface.h"

namespace gsdr_factory
{
// GPU of channel `channel`: `<role>.device` when the configuration sets it, else
// channel % G with G = GNSS-SDR.mi355x_devices (default: every visible device).
// Channels are independent, so this static map is the whole
// multi-GPU scheme: no collective, each GPU ingests the stream for its channels.
int device_for_channel(const ConfigurationInterface* configuration, const std::string& role, int channel);

// nullptr when the implementation name is not an MI355X block (the reference
// factory then falls through to its own switch).
std::unique_ptr<AcquisitionInterface> GetAcqBlock(const ConfigurationInterface* configuration, const std::string& role,
    unsigned int in_streams, unsigned int out_streams, int channel = 0);
std::unique_ptr<TrackingInterface> GetTrkBlock(const ConfigurationInterface* configuration, const std::string& role,
    unsigned int in_streams, unsigned int out_streams, int channel = 0);

// The batched acquisition service (acquisition_service.h) of `signal` -- "1C", "1B"
// or "B1", with the constants of that signal's adapter -- for up to max_requests
// channels reading the device ring `ring` (a DeviceIqRing's stream(); ring_key names
// its input stream) on the ring's device.  With GNSS-SDR.use_acquisition_resampler set and a decimation
// above 1 the service is attached to the process's resampler of (device, ring_key,
// signal) (acq_resampler.h): every service of one signal and stream shares one
// decimated ring, as the reference's channels share one FIR block
// (gnss_flowgraph.cc:1069-1113), and the requests' replicas are sampled at
// service->conf().resampled_fs.  nullptr for another signal.
std::unique_ptr<AcquisitionService> GetAcqService(const ConfigurationInterface* configuration, const std::string& role,
    const std::string& signal, uint32_t max_requests, gsdr_stream* ring, const std::string& ring_key = "rf0",
    uint32_t batch_blocks = 4);
}  // namespace gsdr_factory

#endif
