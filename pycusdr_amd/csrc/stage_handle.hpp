// stage_handle.hpp -- the lifecycle the side handles share (sync finder, combiner, modulator, channel, channeliser, synthesiser):
// each owns a stream and splits its work into begin (enqueue, return) and end (wait, copy out).  Host code only, beside
// hip_owned.hpp; a part of mfbank.hip's one translation unit.  Every piece here serves at least two handles.
//
// What stays with each handle, in its extern "C" functions: the argument and limit checks, in the order that decides the status.
#pragma once
#include <memory>

#include "hip_owned.hpp"
#include "mfb_common.hpp"

// The base of a handle.  It is the FIRST base, so the stream is constructed first and destroyed last: after every buffer and event.
struct StageHandle {
    Stream stream;
    int device = 0;
    Event done;              // recorded behind the work of a begin
    bool busy = false;       // between begin and end

    // high_priority: the sync finder's -- the decoder's small searches run while the demodulator's stream has kernels queued
    int open(bool high_priority) {
        int lo = 0, hi = 0;
        if (high_priority) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIPCHK(high_priority ? hipStreamCreateWithPriority(out(stream), hipStreamNonBlocking, hi)
                             : hipStreamCreateWithFlags(out(stream), hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(out(done), hipEventDisableTiming));
        return MFB_OK;
    }

    // The wait of an end.  With a destination on the host, copy() puts the copies on the stream and the stream is waited for;
    // without one, the event.  Then the handle is free for the next begin.
    template <class Copy>
    int finish(bool to_host, Copy &&copy) {
        if (to_host) {
            HIPCHK(copy());
            HIPCHK(hipStreamSynchronize(stream));
        } else {
            HIPCHK(hipEventSynchronize(done));
        }
        busy = false;
        return MFB_OK;
    }
    // ... of a handle whose begin has already sent the results to its own page-locked staging
    int finish() {
        return finish(false, [] { return hipSuccess; });
    }
};

// Behind every mfb_*_destroy, and the deleter of a create that fails half way.
template <class H>
static int stage_destroy(H *h) {
    if (!h) return MFB_ERR_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return MFB_OK;
}

// Behind every mfb_*_create, after its argument checks: the device check (which makes `device` the current one), then, with no
// exception leaving, a handle with its stream and event, and fill(h) -- the limits and the allocations.  *out only on success.
template <class H, class Fill>
static int stage_create(H **out, int device, Fill &&fill, bool high_priority = false) {
    const int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    return guarded([&]() -> int {
        std::unique_ptr<H, int (*)(H *)> h(new H(), stage_destroy<H>);
        h->device = device;
        int rc2 = h->open(high_priority);
        if (!rc2) rc2 = fill(h.get());
        if (rc2) return rc2;
        *out = h.release();
        return MFB_OK;
    });
}

// The two output sets of channel, channeliser and synthesiser: one is written while the other, finished, is read.
struct OutputSets {
    DevBuf<float2> d_out[2];
    int cur = 0;               // the set of the call in flight
    int count[2] = {0, 0};     // 0: never written

    hipError_t alloc_sets(size_t bytes) {
        hipError_t e = d_out[0].alloc(bytes, dev_alloc);
        return e != hipSuccess ? e : d_out[1].alloc(bytes, dev_alloc);
    }
    // what device_output refuses: the set in flight, and a set never written
    bool readable(bool busy, int buffer) const { return !(busy && cur == buffer) && count[buffer]; }
};

// The timing pair of channeliser and synthesiser: t0 and t1 stand around a call's kernels on the stream.
struct CallTimer {
    Event t0, t1;

    int open_timer() {
        HIPCHK(hipEventCreate(out(t0)));
        HIPCHK(hipEventCreate(out(t1)));
        return MFB_OK;
    }
    // the body of elapsed_ms; ran: a call has finished (each handle's own notion, see profiles/stage_handles.md)
    int elapsed_ms(const StageHandle &h, bool ran, float *ms) const {
        if (h.busy || !ran) return MFB_ERR_STATE;
        HIPCHK(hipSetDevice(h.device));
        HIPCHK(hipEventElapsedTime(ms, t0, t1));
        return MFB_OK;
    }
};

// The sample source of channel and synthesiser: a copy of the host's samples, or the caller's device pointer.
struct SampleSource {
    DevBuf<float2> d_src;
    const float2 *src = nullptr;        // d_src, or the caller's device pointer
    int64_t src_count = 0;

    // The body of set_source, behind the checks.  lazy_samples: where d_src is allocated at the first host source, its samples;
    // 0 where it exists since create.
    int set_source(int device, const void *samples_c64, int64_t nsamples, int on_device, int lazy_samples) {
        HIPCHK(hipSetDevice(device));
        src = nullptr;
        src_count = 0;
        if (on_device) {
            src = (const float2 *)samples_c64;
        } else {
            if (lazy_samples && !d_src) HIPCHK(d_src.alloc((size_t)lazy_samples * sizeof(float2), hip_malloc));
            HIPCHK(hipMemcpy(d_src, samples_c64, (size_t)nsamples * sizeof(float2), hipMemcpyHostToDevice));
            src = d_src;
        }
        src_count = nsamples;
        return MFB_OK;
    }
};
