// Consumer side of the device IQ ring (stream.cpp) for the acquisition and
// tracking translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "gsdr.h"

namespace gsdr
{
int stream_item_type(const gsdr_stream* s);
int stream_device(const gsdr_stream* s);
// GSDR_E_ARG, with the message, unless the ring holds the consumer's item type on its
// device; `who` names the call and `noun` the consumer ("acquisition", "tracking")
int check_ring_consumer(const char* who, const gsdr_stream* ring, int item_type, int device, const char* noun);

// A consumer launch reads the ring under one hold of the ring's lock, from
// choosing its window to recording its reader event, so a push from another
// thread (the GNU Radio producer) cannot land between the two and overwrite the
// window the kernel is about to read: the push waits for the lock, then its copy
// waits for the recorded reader event.
class StreamReader
{
public:
    explicit StreamReader(gsdr_stream* s);
    StreamReader(const StreamReader&) = delete;
    StreamReader& operator=(const StreamReader&) = delete;
    // device pointer of items [first, first + n) (contiguous; checked against the ring)
    int view(uint64_t first, uint64_t n, const void** ptr);
    // the longest contiguous span ending at the head: [*first, *first + *n)
    int span(uint64_t* first, uint64_t* n);
    // make `consumer` wait for the pushes so far
    int acquire(hipStream_t consumer);
    // record the consumer's reads (a push overwriting the oldest item viewed waits for them)
    int release(hipStream_t consumer);
    // the first item ever pushed, the oldest item still held and the head; false before the first push
    bool bounds(uint64_t* base, uint64_t* oldest, uint64_t* head) const;

private:
    gsdr_stream* s_;
    uint64_t lo_{UINT64_MAX};  // the oldest item viewed
    std::unique_lock<std::mutex> lk_;
};

uint64_t stream_capacity(const gsdr_stream* s);
uint64_t stream_window(const gsdr_stream* s);
// the ring is filled by a StreamWriter from now on: gsdr_stream_push is refused
void stream_set_device_produced(gsdr_stream* s);

// Device-side producer of a ring (the decimator, decim.hip): a kernel on the
// ring's own stream writes items [head, head + n) instead of a host push.  The
// ring lock is held from the reservation to the commit, so consumers see either
// the old head or the new one with the `pushed` event recorded behind the kernel.
class StreamWriter
{
public:
    explicit StreamWriter(gsdr_stream* s);
    StreamWriter(const StreamWriter&) = delete;
    StreamWriter& operator=(const StreamWriter&) = delete;
    // the stream the producing kernel is enqueued on
    hipStream_t stream() const;
    uint64_t head() const;
    // items [first, first + n), first == head (the first reservation sets the origin):
    // the producer stream waits for the reader events the items overwrite, as a push
    // does.  The kernel writes item m at ring[m % cap], and at ring[cap + m % cap] too
    // when m % cap < window (the mirror).
    int reserve(uint64_t first, uint64_t n, void** ring, uint64_t* cap, uint64_t* window);
    // after the kernel is enqueued: records `pushed` and advances the head
    int commit();

private:
    gsdr_stream* s_;
    uint64_t reserved_{0};
    std::unique_lock<std::mutex> lk_;
};
}  // namespace gsdr
