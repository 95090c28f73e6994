// channel_api.hpp -- the host side of the channel (mfb_channel_*).
// A part of mfbank.hip's one translation unit: included there once, behind channel_kernels.hpp and stage_handle.hpp.  Host code only.
#pragma once

// ---- the channel (channel_kernels.hpp) ----------------------------------------------------------------------------------------
#define CHAN_MAX_SAMPLES (1 << 24)
#define CHAN_MAX_SOURCE (1 << 26)
#define CHAN_MAX_FRAMES (1 << 20)
static_assert(sizeof(ChanFrame) == sizeof(mfb_channel_frame) && sizeof(ChanFrame) == 48, "the descriptors are copied as they come");
// the output sets: max_samples + 2 each, the aligned pair in front of an odd base, and behind an odd end
struct mfb_channel : StageHandle, OutputSets, SampleSource {
    int max_samples = 0, max_source = 0, max_frames = 0;
    HostBuf<ChanFrame> h_frames;
    DevBuf<ChanFrame> d_frames;
    int64_t base[2] = {0, 0};
};

extern "C" int mfb_channel_destroy(mfb_channel *c) { return stage_destroy(c); }

static int chan_create_impl(mfb_channel *c) {
    HIPCHK(c->h_frames.alloc((size_t)c->max_frames * sizeof(ChanFrame), hip_host_malloc));
    HIPCHK(c->d_frames.alloc((size_t)c->max_frames * sizeof(ChanFrame), dev_alloc));
    HIPCHK(c->alloc_sets(((size_t)c->max_samples + 2) * sizeof(float2)));
    HIPCHK(c->d_src.alloc((size_t)c->max_source * sizeof(float2), dev_alloc));
    return MFB_OK;
}

extern "C" int mfb_channel_create(mfb_channel **out, int device, int max_samples, int max_source, int max_frames) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (max_samples < 1 || max_source < 1 || max_frames < 1) return MFB_ERR_ARG;
    if (max_samples > CHAN_MAX_SAMPLES || max_source > CHAN_MAX_SOURCE || max_frames > CHAN_MAX_FRAMES) return MFB_ERR_UNSUPPORTED;
    return stage_create(out, device, [&](mfb_channel *c) {
        c->max_samples = max_samples;
        c->max_source = max_source;
        c->max_frames = max_frames;
        return chan_create_impl(c);
    });
}

extern "C" int mfb_channel_set_source(mfb_channel *c, const void *samples_c64, int64_t nsamples, int on_device) {
    if (!c || !samples_c64 || nsamples < 1) return MFB_ERR_ARG;
    if (!on_device && nsamples > c->max_source) return MFB_ERR_ARG;
    // (a device pointer's alignment is not looked at here: the synthesiser's set_source does)
    if (c->busy) return MFB_ERR_STATE;
    // not guarded: nothing here allocates -- d_src exists since create (lazy_samples 0)
    return c->set_source(c->device, samples_c64, nsamples, on_device, 0);
}

// a positive, finite power of two whose reciprocal is one too
static bool chan_scale_ok(float s) {
    int e = 0;
    return std::isfinite(s) && s > 0.0f && frexpf(s, &e) == 0.5f && e > -100 && e < 100;
}

static int chan_begin_body(mfb_channel *c, const mfb_channel_params *P, const mfb_channel_frame *frames, int nframes) {
    HIPCHK(hipSetDevice(c->device));
    if (nframes) {
        memcpy(c->h_frames.get(), frames, (size_t)nframes * sizeof(ChanFrame));
        HIPCHK(hipMemcpyAsync(c->d_frames, c->h_frames, (size_t)nframes * sizeof(ChanFrame), hipMemcpyHostToDevice, c->stream));
    }
    ChanArgs A;
    A.base = P->base;
    A.mute_before = P->mute_before;
    A.count = P->count;
    A.nframes = nframes;
    A.key0 = (uint32_t)P->seed;
    A.key1 = (uint32_t)(P->seed >> 32);
    A.sigma = P->sigma;
    A.adc_bits = P->adc_bits;
    A.adc_scale = P->adc_bits ? P->adc_scale : 1.0f;
    A.adc_inv = 1.0f / A.adc_scale;
    const int64_t pairs = ((P->base + P->count + 1) >> 1) - (P->base >> 1);      // <= max_samples / 2 + 1: inside max_samples + 2
    c->count[P->buffer] = 0;
    hipLaunchKernelGGL(k_chan_render, dim3((unsigned)((pairs + CHAN_THREADS - 1) / CHAN_THREADS)), dim3(CHAN_THREADS), 0, c->stream, A,
                       (const ChanFrame *)c->d_frames, c->src, c->d_out[P->buffer].get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->done, c->stream));
    c->cur = P->buffer;
    c->base[P->buffer] = P->base;
    c->count[P->buffer] = P->count;
    c->busy = true;
    return MFB_OK;
}

extern "C" int mfb_channel_begin(mfb_channel *c, const mfb_channel_params *P, const mfb_channel_frame *frames, int nframes) {
    if (!c || !P || nframes < 0 || (nframes > 0 && !frames)) return MFB_ERR_ARG;
    if (P->count < 1 || P->base < 0 || P->mute_before < 0 || (P->buffer != 0 && P->buffer != 1)) return MFB_ERR_ARG;
    if (P->count > CHAN_MAX_SAMPLES || P->base >= ((int64_t)1 << 62) || nframes > CHAN_MAX_FRAMES) return MFB_ERR_UNSUPPORTED;
    if (P->count > c->max_samples || nframes > c->max_frames) return MFB_ERR_ARG;
    if (!std::isfinite(P->sigma) || P->sigma < 0.0f) return MFB_ERR_ARG;
    if (P->adc_bits != 0 && P->adc_bits != 8 && P->adc_bits != 16) return MFB_ERR_ARG;
    if (P->adc_bits && !chan_scale_ok(P->adc_scale)) return MFB_ERR_ARG;
    if (c->busy) return MFB_ERR_STATE;
    if (nframes > 0 && !c->src) return MFB_ERR_STATE;
    int64_t free_from = 0;          // the first position the next frame may take
    for (int f = 0; f < nframes; ++f) {
        const mfb_channel_frame &F = frames[f];
        if (F.length < 1 || F.start < free_from || F.start >= ((int64_t)1 << 62) || !std::isfinite(F.gain)) return MFB_ERR_ARG;
        if (F.src < 0 || F.src > c->src_count - F.length) return MFB_ERR_ARG;
        free_from = F.start + F.length;
    }
    return guarded([&] { return chan_begin_body(c, P, frames, nframes); });
}

extern "C" int mfb_channel_end(mfb_channel *c, float *out_iq) {
    if (!c) return MFB_ERR_ARG;
    if (!c->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const int b = c->cur;
    return c->finish(out_iq != nullptr, [&] {
        return hipMemcpyAsync(out_iq, c->d_out[b].get() + (c->base[b] & 1), (size_t)c->count[b] * sizeof(float2), hipMemcpyDeviceToHost, c->stream);
    });
}

extern "C" int mfb_channel_device_output(mfb_channel *c, int buffer, const void **dev_c64, int64_t *nsamples) {
    if (!c || !dev_c64 || (buffer != 0 && buffer != 1)) return MFB_ERR_ARG;
    if (!c->readable(c->busy, buffer)) return MFB_ERR_STATE;
    *dev_c64 = c->d_out[buffer].get() + (c->base[buffer] & 1);
    if (nsamples) *nsamples = c->count[buffer];
    return MFB_OK;
}

extern "C" int mfb_debug_channel_normals(int device, const uint32_t *words, int npairs, float *out) {
    if (!words || !out || npairs < 1) return MFB_ERR_ARG;
    if (npairs > CHAN_MAX_SAMPLES) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    return guarded([&]() {
        DevBuf<uint32_t> d_w;
        DevBuf<float2> d_o;
        HIPCHK(d_w.alloc((size_t)npairs * 8, hip_malloc));
        HIPCHK(d_o.alloc((size_t)npairs * 8, hip_malloc));
        HIPCHK(hipMemcpy(d_w, words, (size_t)npairs * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_chan_normals, dim3((npairs + 255) / 256), dim3(256), 0, 0, (const uint32_t *)d_w, npairs, d_o.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out, d_o, (size_t)npairs * 8, hipMemcpyDeviceToHost));
        return (int)MFB_OK;
    });
}
