// synthesize_uniform_api.hpp -- the host side of the synthesiser (mfb_synthesizer_*).
// A part of mfbank.hip's one translation unit: included there once, behind synthesize_uniform_kernels.hpp, channelize_api.hpp and stage_handle.hpp.  Host code only.
#pragma once

// ---- the synthesiser (synthesize_uniform_kernels.hpp; channelize_plan.hpp: its limits and the CHZ_SYNTHESIS geometry) --------------
static_assert(sizeof(ChsyPlace) == sizeof(mfb_synthesizer_placement) && sizeof(ChsyPlace) == 32, "the placements are copied as they come");
// d_src: a host source's copy, on demand
struct mfb_synthesizer : StageHandle, OutputSets, CallTimer, SampleSource {
    int M = 0, max_taps = 0, max_out = 0, max_source = 0, max_frames = 0;
    HostBuf<ChsyCall> h_call;  // page-locked staging of a call's table and its sorted placements
    HostBuf<ChsyPlace> h_place;
    DevBuf<ChsyCall> d_call;
    DevBuf<ChsyPlace> d_place;
    DevBuf<float> d_h;
    DevBuf<ChuPlan> d_plan;    // the twiddle table of chu_fft<M>
    bool have_plan = false;
    bool ran = false;          // a call has finished: its time stays readable across a new plan (the channeliser's does not)
    ChzGeom plan = {};         // CHZ_SYNTHESIS
};

extern "C" int mfb_synthesizer_destroy(mfb_synthesizer *s) { return stage_destroy(s); }

static int chsy_create_impl(mfb_synthesizer *s) {
    const int rc = s->open_timer();
    if (rc) return rc;
    HIPCHK(s->h_call.alloc(sizeof(ChsyCall), hip_host_malloc));
    HIPCHK(s->h_place.alloc((size_t)s->max_frames * sizeof(ChsyPlace), hip_host_malloc));
    HIPCHK(s->d_call.alloc(sizeof(ChsyCall), dev_alloc));
    HIPCHK(s->d_place.alloc((size_t)s->max_frames * sizeof(ChsyPlace), dev_alloc));
    HIPCHK(s->d_h.alloc((size_t)s->max_taps * sizeof(float), dev_alloc));
    HIPCHK(s->d_plan.alloc(sizeof(ChuPlan), dev_alloc));
    HIPCHK(s->alloc_sets((size_t)s->max_out * sizeof(float2)));
    ChuPlan P;
    memset(&P, 0, sizeof(P));
    chu_twiddles(s->M, P.tw);
    HIPCHK(hipMemcpy(s->d_plan, &P, sizeof(P), hipMemcpyHostToDevice));
    return MFB_OK;
}

extern "C" int mfb_synthesizer_create(mfb_synthesizer **out, int device, int nbins, int max_taps, int max_out, int max_source, int max_frames) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (nbins < 1 || max_taps < 1 || max_out < 1 || max_source < 1 || max_frames < 1) return MFB_ERR_ARG;
    if (!chu_bins_ok(nbins) || max_taps > CHU_MAX_TAPS || max_out > CHSY_MAX_OUT || max_source > CHSY_MAX_SOURCE || max_frames > CHSY_MAX_FRAMES)
        return MFB_ERR_UNSUPPORTED;
    return stage_create(out, device, [&](mfb_synthesizer *s) {
        s->M = nbins;
        s->max_taps = max_taps;
        s->max_out = max_out;
        s->max_source = max_source;
        s->max_frames = max_frames;
        return chsy_create_impl(s);
    });
}

static int chsy_set_plan_body(mfb_synthesizer *s, const ChzGeom &g, const float *taps) {
    HIPCHK(hipSetDevice(s->device));
    s->have_plan = false;
    HIPCHK(hipMemcpyAsync(s->d_h, taps, (size_t)g.T * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));       // the taps are the caller's
    s->plan = g;
    s->count[0] = s->count[1] = 0;                 // what the sets hold belongs to the plan before
    s->have_plan = true;
    return MFB_OK;
}

extern "C" int mfb_synthesizer_set_plan(mfb_synthesizer *s, int interp, const float *taps, int ntaps) {
    if (!s || !taps || ntaps < 1) return MFB_ERR_ARG;
    if (interp < 2 || interp > s->M || ntaps > CHU_MAX_TAPS) return MFB_ERR_UNSUPPORTED;
    if (ntaps > s->max_taps || !chz_taps_finite(taps, ntaps)) return MFB_ERR_ARG;
    const ChzGeom g = chz_geom(CHZ_SYNTHESIS, interp, 1, ntaps, s->M);
    if (!g.tile) return MFB_ERR_UNSUPPORTED;       // not even one frame's tile fits the LDS budget
    if (s->busy) return MFB_ERR_STATE;
    return guarded([&] { return chsy_set_plan_body(s, g, taps); });
}

extern "C" int mfb_synthesizer_set_source(mfb_synthesizer *s, const void *samples_c64, int64_t nsamples, int on_device) {
    if (!s || !samples_c64 || nsamples < 1) return MFB_ERR_ARG;
    if (!on_device && nsamples > s->max_source) return MFB_ERR_ARG;
    if (on_device && ((uintptr_t)samples_c64 & 7)) return MFB_ERR_ARG;       // (the channel's set_source does not look)
    if (s->busy) return MFB_ERR_STATE;
    // guarded, and d_src allocated at the first host source (lazy_samples = max_source): the channel's is neither
    return guarded([&] { return s->set_source(s->device, samples_c64, nsamples, on_device, s->max_source); });
}

// The call's placements into the staging, sorted by (bin, start), with the table of the occupied bins; false: two of one bin overlap.
static bool chsy_sort_placements(mfb_synthesizer *s, const mfb_synthesizer_placement *pl, int n) {
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return pl[a].bin != pl[b].bin ? pl[a].bin < pl[b].bin : pl[a].start < pl[b].start; });
    ChsyCall &C = *s->h_call.get();
    ChsyPlace *dst = s->h_place.get();
    C.nocc = 0;
    for (int i = 0; i < n; ++i) {
        const mfb_synthesizer_placement &p = pl[order[(size_t)i]];
        if (i && pl[order[(size_t)i - 1]].bin == p.bin) {
            const mfb_synthesizer_placement &before = pl[order[(size_t)i - 1]];
            if (p.start < before.start + before.length) return false;
        } else {
            C.bin[C.nocc] = p.bin;
            C.first[C.nocc++] = i;
        }
        dst[i].start = p.start;
        dst[i].src = p.src;
        dst[i].length = p.length;
        dst[i].bin = p.bin;
        dst[i].gain = p.gain;
        dst[i].reserved = 0;
    }
    C.first[C.nocc] = n;
    return true;
}

static int chsy_begin_body(mfb_synthesizer *s, const mfb_synthesizer_params *p, const mfb_synthesizer_placement *pl, int n) {
    if (!chsy_sort_placements(s, pl, n)) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    const ChzGeom &g = s->plan;
    HIPCHK(hipMemcpyAsync(s->d_call, s->h_call, sizeof(ChsyCall), hipMemcpyHostToDevice, s->stream));
    if (n) HIPCHK(hipMemcpyAsync(s->d_place, s->h_place, (size_t)n * sizeof(ChsyPlace), hipMemcpyHostToDevice, s->stream));
    ChsyArgs A;
    A.out_base = p->out_base;
    A.q_first = p->out_base / g.U;
    A.out_count = p->out_count;
    A.I = g.U;
    A.T = g.T;
    A.J = g.Tb;
    A.F = g.tile;
    A.R = chsy_rows(g.U, g.T, g.tile);
    s->count[p->buffer] = 0;
    HIPCHK(hipEventRecord(s->t0, s->stream));
    visit_chu_bins(g.M, [&](auto m) {
        hipLaunchKernelGGL((k_chsy<decltype(m)::value>), dim3(chsy_grid(g, p->out_base, p->out_count)), dim3(g.threads), g.lds_bytes, s->stream, A,
                           (const ChuPlan *)s->d_plan, (const ChsyCall *)s->d_call, (const ChsyPlace *)s->d_place, s->src, (const float *)s->d_h,
                           s->d_out[p->buffer].get());
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->t1, s->stream));
    HIPCHK(hipEventRecord(s->done, s->stream));
    s->cur = p->buffer;
    s->count[p->buffer] = p->out_count;
    s->busy = true;
    return MFB_OK;
}

extern "C" int mfb_synthesizer_begin(mfb_synthesizer *s, const mfb_synthesizer_params *p, const mfb_synthesizer_placement *pl, int n) {
    if (!s || !p || n < 0 || (n > 0 && !pl)) return MFB_ERR_ARG;
    if (p->out_count < 1 || p->out_base < 0 || (p->buffer != 0 && p->buffer != 1)) return MFB_ERR_ARG;
    if (p->out_count > CHSY_MAX_OUT || p->out_base >= ((int64_t)1 << 62) || n > CHSY_MAX_FRAMES) return MFB_ERR_UNSUPPORTED;
    if (p->out_count > s->max_out || n > s->max_frames) return MFB_ERR_ARG;
    if (s->busy || !s->have_plan || !s->src) return MFB_ERR_STATE;
    for (int i = 0; i < n; ++i) {
        const mfb_synthesizer_placement &q = pl[i];
        if (q.length < 1 || q.start < 0 || q.bin < 0 || q.bin >= s->M || !std::isfinite(q.gain)) return MFB_ERR_ARG;
        if (q.start >= ((int64_t)1 << 62)) return MFB_ERR_UNSUPPORTED;
        if (q.src < 0 || q.src > s->src_count - q.length) return MFB_ERR_ARG;
    }
    return guarded([&] { return chsy_begin_body(s, p, pl, n); });
}

extern "C" int mfb_synthesizer_end(mfb_synthesizer *s, float *out_c64) {
    if (!s) return MFB_ERR_ARG;
    if (!s->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(s->device));
    const int rc = s->finish(out_c64 != nullptr, [&] {
        return hipMemcpyAsync(out_c64, s->d_out[s->cur], (size_t)s->count[s->cur] * sizeof(float2), hipMemcpyDeviceToHost, s->stream);
    });
    if (rc) return rc;
    s->ran = true;
    return MFB_OK;
}

extern "C" int mfb_synthesizer_device_output(mfb_synthesizer *s, int buffer, const void **dev_c64, int64_t *nsamples) {
    if (!s || !dev_c64 || (buffer != 0 && buffer != 1)) return MFB_ERR_ARG;
    if (!s->readable(s->busy, buffer)) return MFB_ERR_STATE;
    *dev_c64 = s->d_out[buffer].get();
    if (nsamples) *nsamples = s->count[buffer];
    return MFB_OK;
}

extern "C" int mfb_synthesizer_info(mfb_synthesizer *s, int *frames_per_workgroup, int *rows) {
    if (!s) return MFB_ERR_ARG;
    if (!s->have_plan) return MFB_ERR_STATE;
    if (frames_per_workgroup) *frames_per_workgroup = s->plan.tile;
    if (rows) *rows = chsy_rows(s->plan.U, s->plan.T, s->plan.tile);
    return MFB_OK;
}

extern "C" int mfb_synthesizer_elapsed_ms(mfb_synthesizer *s, float *ms) {
    if (!s || !ms) return MFB_ERR_ARG;
    return s->elapsed_ms(*s, s->ran, ms);
}
