// bank_input_api.hpp -- where a bank's samples arrive: sample formats and k_unpack, the page-locked inputs and windows, input_copy.
// A part of mfbank.hip's one translation unit: included there once, behind bank_ctx.hpp.  Host code only.
#pragma once

// ---- integer IQ samples (unpack_kernels.hpp) ---------------------------------------------------------------------------------
// The value of one integer step: 0 = full scale 1.0 (2^-15 / 2^-7), else a positive power of two that keeps every product a normal
// float -- the whole reason the conversion is exact (include/mfbank.h).  Returns 0 for anything else.
static float fmt_scale_checked(int fmt, float scale) {
    if (scale == 0.f) return fmt == MFB_SAMPLES_SC16 ? 0x1p-15f : 0x1p-7f;
    int e = 0;
    if (!(scale > 0.f) || isinf(scale) || frexpf(scale, &e) != 0.5f) return 0.f;
    const float top = scale * (fmt == MFB_SAMPLES_SC16 ? 32768.f : 128.f);
    if (scale < 0x1p-126f || isinf(top)) return 0.f;
    return scale;
}
static int launch_unpack(int fmt, const void *raw, cf *dst, size_t samples, float scale, hipStream_t s) {
    const dim3 grid((unsigned)unpack_blocks(fmt, samples)), block(UNPACK_THREADS);
    if (fmt == MFB_SAMPLES_SC16) hipLaunchKernelGGL(k_unpack<UNPACK_SC16>, grid, block, 0, s, raw, (float2 *)dst, samples, scale);
    else hipLaunchKernelGGL(k_unpack<UNPACK_SC8>, grid, block, 0, s, raw, (float2 *)dst, samples, scale);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}
// `samples` raw samples of a page-locked input to its staging buffer `rawslot` and, right behind the copy on the same stream,
// as complex64 into dst.  The staging buffer is made (or grown: everything that may read the old one is waited for) here.
static int raw_copy_unpack(mfb_ctx *c, const void *src, cf *dst, size_t samples, int rawslot, hipStream_t s) {
    const size_t bytes = samples * (size_t)sample_bytes(c->fmt), need = (bytes + 15) & ~(size_t)15;
    if (c->raw_cap[rawslot] < need) {
        if (c->d_raw[rawslot]) {
            HIPCHK(sync_streams(c));
            if (c->in_stream) HIPCHK(hipStreamSynchronize(c->in_stream));
        }
        const int rc = grow_buffers(&c->raw_cap[rawslot], need, {{&c->d_raw[rawslot], need}});
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(c->d_raw[rawslot], src, bytes, hipMemcpyHostToDevice, s));
    return launch_unpack(c->fmt, c->d_raw[rawslot], dst, samples, c->fmt_scale, s);
}

extern "C" int mfb_input_buffer(mfb_ctx *c, float **p) {
    if (!c || !p) return MFB_ERR_ARG;
    if (c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the buffer holds integers: mfb_input_buffer_raw
    *p = (float *)c->h_in.get();
    return MFB_OK;
}

static int input_buffer2(mfb_ctx *c) {
    if (!c->h_in2) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(c->h_in2.alloc((size_t)c->N * sizeof(cf), hip_host_malloc));
        memset(c->h_in2, 0, (size_t)c->N * sizeof(cf));
        if (!c->d_x2) HIPCHK(c->d_x2.alloc((size_t)c->N * sizeof(cf), dev_alloc));
    }
    return MFB_OK;
}
extern "C" int mfb_input_buffer2(mfb_ctx *c, float **p) {
    if (!c || !p) return MFB_ERR_ARG;
    if (c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the buffer holds integers: mfb_input_buffer_raw
    const int rc = input_buffer2(c);
    if (rc) return rc;
    *p = (float *)c->h_in2.get();
    return MFB_OK;
}
extern "C" int mfb_input_buffer_raw(mfb_ctx *c, int which, void **host, size_t *bytes) {
    if (!c || !host || !bytes || which < 0 || which > 1) return MFB_ERR_ARG;
    if (which) {
        const int rc = input_buffer2(c);
        if (rc) return rc;
    }
    *host = which ? c->h_in2 : c->h_in;
    *bytes = (size_t)c->N * (size_t)sample_bytes(c->fmt);
    return MFB_OK;
}

// Host-to-device copy of a page-locked input buffer into its own device copy, on the input stream: it starts as soon as the
// last block that read that device copy is done -- i.e. while the block before this one is still being searched -- and the
// handle's stream picks it up with an event.  (With one device buffer and one stream the copy of an 8 MiB block, 0.15 ms,
// sat between two searches.)
// Under an integer sample format (mfb_set_sample_format) the raw bytes go to the input's staging buffer `rawslot` and k_unpack
// writes the complex64 device copy right behind the copy, on the input stream too: whatever waits for the event reads what it
// always read.  (Copy and unpack stay outside the recorded graphs, which begin behind that event.)
static int input_copy(mfb_ctx *c, const cf *src, cf *dst, size_t samples, Event *ev_h2d, Event *ev_free, int which, int rawslot) {
    if (!src || !dst) return MFB_ERR_STATE;
    if (!c->in_stream) HIPCHK(hipStreamCreateWithFlags(out(c->in_stream), hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (!ev_h2d[i]) HIPCHK(hipEventCreateWithFlags(out(ev_h2d[i]), hipEventDisableTiming));
        if (!ev_free[i]) {
            HIPCHK(hipEventCreateWithFlags(out(ev_free[i]), hipEventDisableTiming));
            HIPCHK(hipEventRecord(ev_free[i], c->stream));
        }
    }
    HIPCHK(hipStreamWaitEvent(c->in_stream, ev_free[which], 0));
    if (c->fmt != MFB_SAMPLES_CF32) {
        const int rc = raw_copy_unpack(c, src, dst, samples, rawslot, c->in_stream);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(dst, src, samples * sizeof(cf), hipMemcpyHostToDevice, c->in_stream));
    }
    HIPCHK(hipEventRecord(ev_h2d[which], c->in_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, ev_h2d[which], 0));
    return MFB_OK;
}
static int block_input_copy(mfb_ctx *c, int which) {
    return input_copy(c, which ? c->h_in2 : c->h_in, which ? c->d_x2 : c->d_x, (size_t)c->N, c->ev_h2d, c->ev_xfree, which, which);
}

// ---- B consecutive blocks per call ---------------------------------------------------------------------------------------
// The reference's own configurations use blocks of 2^15 ... 2^17 samples with 64 bins (config/base.json:13,33): one such block
// is a few tens of microseconds of device work, and a loop that hands the device one block per turn (DP:284-338) leaves it idle
// most of the time.  Here B consecutive blocks of the stream go to the device as ONE contiguous window of
// B * stride + (N - stride) samples (stride = N - overlap: block b starts at b * stride -- the overlap between neighbours is
// shared storage, nothing is copied twice) and through ONE set of launches: batched forward FFT, one search launch over
// B x D (block, bin) streams, B picks in one launch, one matched-filter launch at the B shifts, batched envelope FFT, B rate
// estimates, the centres of all blocks, one device-to-host copy of B result records.
static int window_samples(const mfb_ctx *c, int nb) { return nb * c->win_stride + (c->N - c->win_stride); }

static int window_buffer(mfb_ctx *c, int which, int max_blocks, int block_stride, void **host_c64) {
    if (!c || !host_c64 || which < 0 || which > 1 || max_blocks < 1 || max_blocks > 1024 || block_stride < 1 || block_stride > c->N)
        return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->win_blocks != max_blocks || c->win_stride != block_stride) {
        for (int s = 0; s < 2; ++s)
            if (c->flight[s].active && c->flight[s].nb) return MFB_ERR_STATE;      // a batch is reading the windows
        HIPCHK(sync_and_invalidate(c, true));
        for (int i = 0; i < 2; ++i) {
            c->raw_cap[2 + i] = 0;
            HIPCHK(c->h_win[i].reset());
            HIPCHK(c->d_win[i].reset());
            HIPCHK(c->d_raw[2 + i].reset());
        }
        c->win_blocks = max_blocks;
        c->win_stride = block_stride;
    }
    if (!c->h_win[which]) {
        const size_t bytes = (size_t)window_samples(c, c->win_blocks) * sizeof(cf);
        HIPCHK(c->h_win[which].alloc(bytes, hip_host_malloc));
        memset(c->h_win[which], 0, bytes);
        HIPCHK(c->d_win[which].alloc(bytes, dev_alloc));
    }
    *host_c64 = c->h_win[which];
    return MFB_OK;
}
extern "C" int mfb_window_buffer(mfb_ctx *c, int which, int max_blocks, int block_stride, float **host_c64) {
    if (c && c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the windows hold integers: mfb_window_buffer_raw
    void *p = nullptr;
    const int rc = window_buffer(c, which, max_blocks, block_stride, host_c64 ? &p : nullptr);
    if (!rc) *host_c64 = (float *)p;
    return rc;
}
extern "C" int mfb_window_buffer_raw(mfb_ctx *c, int which, int max_blocks, int block_stride, void **host, size_t *bytes) {
    if (!bytes) return MFB_ERR_ARG;
    const int rc = window_buffer(c, which, max_blocks, block_stride, host);
    if (!rc) *bytes = (size_t)window_samples(c, c->win_blocks) * (size_t)sample_bytes(c->fmt);
    return rc;
}

extern "C" int mfb_set_sample_format(mfb_ctx *c, int format, float scale) {
    if (!c || (format != MFB_SAMPLES_CF32 && format != MFB_SAMPLES_SC16 && format != MFB_SAMPLES_SC8)) return MFB_ERR_ARG;
    float sc = 1.f;
    if (format == MFB_SAMPLES_CF32) {
        if (scale != 0.f && scale != 1.f) return MFB_ERR_ARG;      // complex64 is taken as it is
    } else if ((sc = fmt_scale_checked(format, scale)) == 0.f) {
        return MFB_ERR_ARG;
    }
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_and_invalidate(c, true));        // no recorded graph outlives the element type of its input
    c->fmt = format;
    c->fmt_scale = sc;
    c->clip_restart = true;      // the chain's tail belongs to samples of the other type's stream
    // what the buffers held means nothing as the new type
    if (c->h_in) memset(c->h_in, 0, (size_t)c->N * sizeof(cf));
    if (c->h_in2) memset(c->h_in2, 0, (size_t)c->N * sizeof(cf));
    for (int i = 0; i < 2; ++i)
        if (c->h_win[i]) memset(c->h_win[i], 0, (size_t)window_samples(c, c->win_blocks) * sizeof(cf));
    return MFB_OK;
}
extern "C" int mfb_get_sample_format(mfb_ctx *c, int *format, float *scale, int *bytes_per_sample) {
    if (!c) return MFB_ERR_ARG;
    if (format) *format = c->fmt;
    if (scale) *scale = c->fmt_scale;
    if (bytes_per_sample) *bytes_per_sample = (int)sample_bytes(c->fmt);
    return MFB_OK;
}
