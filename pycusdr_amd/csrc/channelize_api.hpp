// channelize_api.hpp -- the host side of the channeliser (mfb_channelizer_*): the five kinds of plan and the survey.
// A part of mfbank.hip's one translation unit: included there once, behind the channelize_*_kernels.hpp and channelize_plan.hpp and stage_handle.hpp.  Host code only.
#pragma once

// ---- the channeliser (channelize_plan.hpp: the limits and what a plan of each kind launches; the kernels: channelize_kernels.hpp,
// channelize_rational_kernels.hpp, channelize_uniform_kernels.hpp, channelize_uniform_rational_kernels.hpp,
// channelize_survey_kernels.hpp) -----------------------------------------------------------------------------------------------
// the output sets: [max_channels][out_stride] each
struct mfb_channelizer : StageHandle, OutputSets, CallTimer {
    int max_channels = 0, max_taps = 0, max_in = 0, max_out = 0;
    int M = 0;                 // the bins of a handle made by mfb_channelizer_create_uniform, which takes plans of
                               // mfb_channelizer_set_plan_uniform and mfb_uniform_channelizer_set_plan_rational only; 0: mfb_channelizer_create
    int out_stride = 0;        // float2 between two channels of an output set: max_out made even, so every channel is 16-byte aligned
    HostBuf<uint8_t> h_in[2];  // page-locked raw staging, on demand (mfb_channelizer_input_buffer)
    DevBuf<uint8_t> d_in[2];   // their device copies, on demand
    DevBuf<float> d_h;
    DevBuf<ChzPlan> d_plan;
    DevBuf<float2> d_taps;     // [max_channels][max_taps]
    DevBuf<float2> d_rtaps;    // a rational plan's tables by branch, [max_channels][rtap_stride], on demand
    bool have_plan = false;
    ChzGeom plan = {};         // what a call of the plan in force launches; its kind says which kernel
    ChzGeom survey = {};       // what a survey call of a uniform plan launches (CHZ_SURVEY)
    int K = 0, fmt = 0, ncplx = 0;
    int rtap_stride = 0;       // max_taps + CHZR_MAX_INTERP - 1 >= U Tb
    DevBuf<ChuPlan> d_uplan;   // a uniform handle's twiddle table and the selected bins' columns
    DevBuf<float> d_ubr;       // a uniform rational plan's taps by branch, [U][ceil(T / U)] within CHZR_MAX_INTERP max_taps, on demand
    float scale = 1.0f;
    int nchan[2] = {0, 0};     // the plan's channels when a set was written
    // the survey of a uniform plan (mfb_channelizer_set_survey)
    int sv_L = 0;              // frames per cell; 0: no survey set
    int sv_rank = 0;
    float sv_thr = 0.0f;
    DevBuf<float> d_svpart;    // [chunks][M]
    DevBuf<float> d_svpower;   // [cells][M]
    DevBuf<float> d_svfloor;   // [cells]
    DevBuf<uint32_t> d_svmask; // [cells][ceil(M / 32)]
    bool sv_call = false;      // the call in flight, or finished last, came from mfb_channelizer_survey_begin
    bool sv_wrote = false;     // and wrote its output set
    int sv_cells = 0;          // its cells
};

extern "C" int mfb_channelizer_destroy(mfb_channelizer *c) { return stage_destroy(c); }

static int chz_create_impl(mfb_channelizer *c) {
    const int rc = c->open_timer();
    if (rc) return rc;
    HIPCHK(c->d_h.alloc((size_t)c->max_taps * sizeof(float), dev_alloc));
    if (c->M) {
        HIPCHK(c->d_uplan.alloc(sizeof(ChuPlan), dev_alloc));
    } else {
        HIPCHK(c->d_plan.alloc(sizeof(ChzPlan), dev_alloc));
        HIPCHK(c->d_taps.alloc((size_t)c->max_channels * c->max_taps * sizeof(float2), dev_alloc));
    }
    HIPCHK(c->alloc_sets((size_t)c->max_channels * c->out_stride * sizeof(float2)));
    return MFB_OK;
}

// behind the argument checks of either create; nbins: 0 for mfb_channelizer_create
static int chz_create(mfb_channelizer **out, int device, int nbins, int max_channels, int max_taps, int max_in, int max_out) {
    return stage_create(out, device, [&](mfb_channelizer *c) {
        c->M = nbins;
        c->max_channels = max_channels;
        c->max_taps = max_taps;
        c->max_in = max_in;
        c->max_out = max_out;
        c->out_stride = (max_out + 1) & ~1;
        return chz_create_impl(c);
    });
}

extern "C" int mfb_channelizer_create(mfb_channelizer **out, int device, int max_channels, int max_taps, int max_in, int max_out) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (max_channels < 1 || max_taps < 1 || max_in < 1 || max_out < 1) return MFB_ERR_ARG;
    if (max_channels > CHZ_MAX_CHANNELS || max_taps > CHZ_MAX_TAPS || max_in > CHZ_MAX_IN || max_out > CHZ_MAX_OUT) return MFB_ERR_UNSUPPORTED;
    return chz_create(out, device, 0, max_channels, max_taps, max_in, max_out);
}

static bool chu_bins_ok(int M) { return M == 8 || M == 16 || M == 32 || M == 64 || M == 128 || M == 256; }

extern "C" int mfb_channelizer_create_uniform(mfb_channelizer **out, int device, int nbins, int max_selected, int max_taps, int max_in,
                                              int max_out) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (nbins < 1 || max_selected < 1 || max_taps < 1 || max_in < 1 || max_out < 1) return MFB_ERR_ARG;
    if (!chu_bins_ok(nbins) || max_selected > nbins || max_taps > CHU_MAX_TAPS || max_in > CHZ_MAX_IN || max_out > CHZ_MAX_OUT)
        return MFB_ERR_UNSUPPORTED;
    if ((int64_t)max_selected * max_out > CHU_MAX_SET) return MFB_ERR_UNSUPPORTED;
    return chz_create(out, device, nbins, max_selected, max_taps, max_in, max_out);
}

// What every set_plan refuses, in the order of the codes: `which` are the plan's n tuning words or selected bins; kind_tests() the
// limits and the arguments of the one kind of plan, MFB_ERR_UNSUPPORTED before MFB_ERR_ARG.  *scale: the scale the plan runs with.
// branch_interp: the U of a rational plan on the raster, whose handle holds max_taps taps per branch; 1 for every other kind.
template <class KindTests>
static int chz_plan_check(mfb_channelizer *c, bool uniform, const float *taps, int ntaps, const void *which, int n, int fmt, float sample_scale,
                          float *scale, KindTests kind_tests, int branch_interp = 1) {
    if (!c || !taps || !which || ntaps < 1 || n < 1) return MFB_ERR_ARG;
    if ((c->M != 0) != uniform) return MFB_ERR_STATE;
    if (!chz_format_ok(fmt)) return MFB_ERR_ARG;
    const int rc = kind_tests();
    if (rc) return rc;
    if (chzr_branch_taps(branch_interp, ntaps) > c->max_taps || n > c->max_channels) return MFB_ERR_ARG;
    if (!chz_plan_scale(fmt, sample_scale, chan_scale_ok, scale) || !chz_taps_finite(taps, ntaps)) return MFB_ERR_ARG;
    return c->busy ? MFB_ERR_STATE : MFB_OK;
}

// The plan's taps and table are on their way on the stream: wait for them (both are the caller's, or the caller's frame's), then
// the plan is in force.  Until here a set_plan that fails leaves the handle without a plan.
static int chz_plan_commit(mfb_channelizer *c, const ChzGeom &g, int K, int ncplx, int fmt, float scale) {
    HIPCHK(hipStreamSynchronize(c->stream));
    c->plan = g;
    c->K = K;
    c->ncplx = ncplx;
    c->fmt = fmt;
    c->scale = scale;
    c->count[0] = c->count[1] = 0;                 // what the buffers hold belongs to the plan before
    c->have_plan = true;
    return MFB_OK;
}

static int chz_set_plan_body(mfb_channelizer *c, const ChzGeom &g, const float *taps, const uint64_t *freq_words, int nchan, int fmt,
                             float scale) {
    HIPCHK(hipSetDevice(c->device));
    if (g.kind == CHZ_RATIONAL && !c->d_rtaps) {
        c->rtap_stride = c->max_taps + CHZR_MAX_INTERP - 1;
        HIPCHK(c->d_rtaps.alloc((size_t)c->max_channels * c->rtap_stride * sizeof(float2), hip_malloc));
    }
    ChzPlan P;
    memset(&P, 0, sizeof(P));
    int ncplx = 0, at = 0;
    for (int k = 0; k < nchan; ++k) {
        P.freq[k] = freq_words[k];
        if (freq_words[k] != 0) P.order[ncplx++] = k;
    }
    at = ncplx;
    for (int k = 0; k < nchan; ++k)
        if (freq_words[k] == 0) P.order[at++] = k;
    c->have_plan = false;
    HIPCHK(hipMemcpyAsync(c->d_h, taps, (size_t)g.T * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_plan, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    if (g.kind == CHZ_RATIONAL)
        hipLaunchKernelGGL(k_chzr_taps, dim3((g.U * g.Tb + 255) / 256, nchan), dim3(256), 0, c->stream, (const float *)c->d_h,
                           (const ChzPlan *)c->d_plan, g.U, g.T, g.Tb, c->rtap_stride, c->d_rtaps.get());
    else
        hipLaunchKernelGGL(k_chz_taps, dim3((g.T + 255) / 256, nchan), dim3(256), 0, c->stream, (const float *)c->d_h, (const ChzPlan *)c->d_plan,
                           g.T, c->max_taps, c->d_taps.get());
    HIPCHK(hipGetLastError());
    return chz_plan_commit(c, g, nchan, ncplx, fmt, scale);
}

// kind: CHZ_INTEGER (interp 1) or CHZ_RATIONAL, which runs k_chzr also at U = 1
static int chz_set_plan(mfb_channelizer *c, int kind, int interp, int decim, const float *taps, int ntaps, const uint64_t *freq_words, int nchan,
                        int sample_format, float sample_scale) {
    float scale = 1.0f;
    const int rc = chz_plan_check(c, false, taps, ntaps, freq_words, nchan, sample_format, sample_scale, &scale, [&]() -> int {
        if (decim < 2 || decim > CHZ_MAX_DECIM || ntaps > CHZ_MAX_TAPS || nchan > CHZ_MAX_CHANNELS) return MFB_ERR_UNSUPPORTED;
        if (interp < 1 || interp > CHZR_MAX_INTERP) return MFB_ERR_UNSUPPORTED;
        if (interp >= decim || ntaps < interp || !chzr_coprime(interp, decim)) return MFB_ERR_ARG;
        return MFB_OK;
    });
    if (rc) return rc;
    return guarded([&] { return chz_set_plan_body(c, chz_geom(kind, interp, decim, ntaps, 0), taps, freq_words, nchan, sample_format, scale); });
}

extern "C" int mfb_channelizer_set_plan(mfb_channelizer *c, int decim, const float *taps, int ntaps, const uint64_t *freq_words, int nchan,
                                        int sample_format, float sample_scale) {
    return chz_set_plan(c, CHZ_INTEGER, 1, decim, taps, ntaps, freq_words, nchan, sample_format, sample_scale);
}

extern "C" int mfb_channelizer_set_plan_rational(mfb_channelizer *c, int interp, int decim, const float *taps, int ntaps,
                                                 const uint64_t *freq_words, int nchan, int sample_format, float sample_scale) {
    return chz_set_plan(c, CHZ_RATIONAL, interp, decim, taps, ntaps, freq_words, nchan, sample_format, sample_scale);
}

static hipError_t chus_drop(mfb_channelizer *c) {
    c->sv_L = 0;
    c->sv_call = false;
    hipError_t e = c->d_svpart.reset(), e2;
    if ((e2 = c->d_svpower.reset()) != hipSuccess) e = e2;
    if ((e2 = c->d_svfloor.reset()) != hipSuccess) e = e2;
    if ((e2 = c->d_svmask.reset()) != hipSuccess) e = e2;
    return e;
}

// e^{2 pi i q / M}, q < M, of chu_fft<M> (also the synthesiser's)
static void chu_twiddles(int M, float2 *tw) {
    for (int q = 0; q < M; ++q) {                    // rounded once from float64; the multiples of a quarter turn are exact
        const int e = q % (M / 4), quad = q / (M / 4);
        double re = 1.0, im = 0.0;
        if (e) {
            const double a = 2.0 * M_PI * (double)e / (double)M;
            re = cos(a);
            im = sin(a);
        }
        for (int i = 0; i < quad; ++i) {             // times i
            const double t = re;
            re = -im;
            im = t;
        }
        tw[q] = make_float2((float)re, (float)im);
    }
}

// kind: CHZ_UNIFORM (interp 1) or CHZ_UNIFORM_RATIONAL, which runs k_chur also at U = 1
static int chu_set_plan_body(mfb_channelizer *c, int kind, int interp, int decim, const float *taps, int ntaps, const int32_t *bins, int nsel,
                             int fmt, float scale) {
    HIPCHK(hipSetDevice(c->device));
    ChuPlan P;
    memset(&P, 0, sizeof(P));
    const int M = c->M;
    chu_twiddles(M, P.tw);
    for (int i = 0; i < nsel; ++i) P.col[i] = chu_column(M, bins[i]);
    const ChzGeom g = chz_geom(kind, interp, decim, ntaps, M);
    std::vector<float> branches;                   // [r][j] = h[r + j U], rows of Tb; 0, never read, where r + j U >= T
    c->have_plan = false;
    HIPCHK(chus_drop(c));                          // a survey belongs to the plan it was set under
    if (kind == CHZ_UNIFORM_RATIONAL) {
        if (!c->d_ubr) HIPCHK(c->d_ubr.alloc((size_t)CHZR_MAX_INTERP * c->max_taps * sizeof(float), hip_malloc));
        branches.assign((size_t)g.U * g.Tb, 0.0f);
        for (int t = 0; t < ntaps; ++t) branches[(size_t)(t % g.U) * g.Tb + t / g.U] = taps[t];
        HIPCHK(hipMemcpyAsync(c->d_ubr, branches.data(), branches.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->survey = {};                            // the survey is a matter of integer plans
    } else {
        HIPCHK(hipMemcpyAsync(c->d_h, taps, (size_t)ntaps * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->survey = chz_geom(CHZ_SURVEY, 1, decim, ntaps, M);
    }
    HIPCHK(hipMemcpyAsync(c->d_uplan, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    return chz_plan_commit(c, g, nsel, 0, fmt, scale);                           // (waits: `branches` and P have been read)
}

// MFB_ERR_ARG for a selected bin outside [0, M) or named twice
static int chu_bins_check(const mfb_channelizer *c, const int32_t *bins, int nselected) {
    bool seen[CHU_MAX_BINS] = {};
    for (int i = 0; i < nselected; ++i) {
        if (bins[i] < 0 || bins[i] >= c->M || seen[bins[i]]) return MFB_ERR_ARG;
        seen[bins[i]] = true;
    }
    return MFB_OK;
}

extern "C" int mfb_channelizer_set_plan_uniform(mfb_channelizer *c, int decim, const float *taps, int ntaps, const int32_t *bins, int nselected,
                                                int sample_format, float sample_scale) {
    float scale = 1.0f;
    const int rc = chz_plan_check(c, true, taps, ntaps, bins, nselected, sample_format, sample_scale, &scale, [&]() -> int {
        if (decim < 2 || decim > c->M || ntaps > CHU_MAX_TAPS || nselected > c->M) return MFB_ERR_UNSUPPORTED;
        return chu_bins_check(c, bins, nselected);
    });
    if (rc) return rc;
    return guarded([&] { return chu_set_plan_body(c, CHZ_UNIFORM, 1, decim, taps, ntaps, bins, nselected, sample_format, scale); });
}

extern "C" int mfb_uniform_channelizer_set_plan_rational(mfb_channelizer *c, int interp, int decim, const float *taps, int ntaps,
                                                         const int32_t *bins, int nselected, int sample_format, float sample_scale) {
    float scale = 1.0f;
    const int rc = chz_plan_check(
        c, true, taps, ntaps, bins, nselected, sample_format, sample_scale, &scale,
        [&]() -> int {
            if (interp < 1 || interp > CHZR_MAX_INTERP || decim < 2 || decim > interp * c->M || nselected > c->M) return MFB_ERR_UNSUPPORTED;
            if (chzr_branch_taps(interp, ntaps) > CHU_MAX_TAPS) return MFB_ERR_UNSUPPORTED;
            if (c->sv_L) return MFB_ERR_UNSUPPORTED;                             // a survey is set: it stays with integer plans
            if (interp >= decim || ntaps < interp || !chzr_coprime(interp, decim)) return MFB_ERR_ARG;
            return chu_bins_check(c, bins, nselected);
        },
        interp);
    if (rc) return rc;
    return guarded(
        [&] { return chu_set_plan_body(c, CHZ_UNIFORM_RATIONAL, interp, decim, taps, ntaps, bins, nselected, sample_format, scale); });
}

extern "C" int mfb_channelizer_input_buffer(mfb_channelizer *c, int which, void **host, size_t *bytes) {
    if (!c || !host || (which != 0 && which != 1)) return MFB_ERR_ARG;
    if (!c->have_plan) return MFB_ERR_STATE;
    return guarded([&]() {          // (also while a call is in flight: the other buffer is being filled)
        HIPCHK(hipSetDevice(c->device));
        if (!c->h_in[which]) HIPCHK(c->h_in[which].alloc((size_t)c->max_in * sizeof(float2), hip_host_malloc));
        *host = c->h_in[which].get();
        if (bytes) *bytes = (size_t)c->max_in * sample_bytes(c->fmt);
        return (int)MFB_OK;
    });
}

extern "C" int mfb_channelizer_info(mfb_channelizer *c, int *outputs_per_workgroup, int *taps_capacity) {
    if (!c) return MFB_ERR_ARG;
    if (!c->have_plan) return MFB_ERR_STATE;
    if (outputs_per_workgroup) *outputs_per_workgroup = c->plan.tile;
    if (taps_capacity) *taps_capacity = c->max_taps;
    return MFB_OK;
}

// ---- the launches: one function per kind of plan
// f(tag) with tag::value the CHZ_FMT_* of the plan's sample format / the bins of a uniform handle: the kernels' template arguments
template <class F>
static void visit_chz_fmt(int fmt, F f) {
    if (fmt == MFB_SAMPLES_SC16) f(std::integral_constant<int, CHZ_FMT_SC16>{});
    else if (fmt == MFB_SAMPLES_SC8) f(std::integral_constant<int, CHZ_FMT_SC8>{});
    else f(std::integral_constant<int, CHZ_FMT_CF32>{});
}
template <class F>
static void visit_chu_bins(int M, F f) {
    switch (M) {
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 128: f(std::integral_constant<int, 128>{}); break;
        default: f(std::integral_constant<int, 256>{}); break;
    }
}

// the call's window and the plan's D, T, scale: the fields that ChzArgs, ChzrArgs and ChuArgs share
template <class Args>
static Args chz_window(const mfb_channelizer *c, const ChzGeom &g, const mfb_channelizer_params *p) {
    Args A;
    A.in_base = p->in_base;
    A.in_end = p->in_base + p->in_count;
    A.out_base = p->out_base;
    A.out_count = p->out_count;
    A.D = g.D;
    A.T = g.T;
    A.out_stride = c->out_stride;
    A.scale = c->scale;
    return A;
}

static void chu_launch(mfb_channelizer *c, const mfb_channelizer_params *p, const void *raw) {
    const ChzGeom &g = c->plan;
    ChuArgs A = chz_window<ChuArgs>(c, g, p);
    A.F = g.tile;
    A.nsel = c->K;
    visit_chu_bins(g.M, [&](auto m) {
        visit_chz_fmt(c->fmt, [&](auto fmt) {
            hipLaunchKernelGGL((k_chu<decltype(m)::value, decltype(fmt)::value>), dim3(chz_grid(g, p->out_count)), dim3(g.threads), g.lds_bytes,
                               c->stream, A, (const ChuPlan *)c->d_uplan, raw, (const float *)c->d_h, c->d_out[p->buffer].get());
        });
    });
}

// U / gcd(U, 256 / M): frames that far apart in a lane's walk share a branch (channelize_uniform_rational_kernels.hpp)
static int chur_share(int U, int M) {
    int a = U, b = CHU_THREADS / M;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    return U / a;
}

static void chur_launch(mfb_channelizer *c, const mfb_channelizer_params *p, const void *raw) {
    const ChzGeom &g = c->plan;
    ChurArgs A = chz_window<ChurArgs>(c, g, p);
    A.U = g.U;
    A.Tb = g.Tb;
    A.F = g.tile;
    A.nsel = c->K;
    A.span = g.S;
    A.share = chur_share(g.U, g.M);
    const int step = (CHU_THREADS / g.M) * g.D;                   // positions at the virtual rate between two frames of a lane's walk
    A.share_dq = A.share * step / g.U;                            // exact: share (256 / M) is a multiple of U
    A.step_dq = step / g.U;
    A.step_r = step % g.U;
    visit_chu_bins(g.M, [&](auto m) {
        visit_chz_fmt(c->fmt, [&](auto fmt) {
            hipLaunchKernelGGL((k_chur<decltype(m)::value, decltype(fmt)::value>), dim3(chz_grid(g, p->out_count)), dim3(g.threads), g.lds_bytes,
                               c->stream, A, (const ChuPlan *)c->d_uplan, raw, (const float *)c->d_ubr, c->d_out[p->buffer].get());
        });
    });
}

// the survey kernel, with or without the store, and the finishing kernel behind it
static void chus_launch(mfb_channelizer *c, const mfb_channelizer_params *p, const void *raw, bool write) {
    const ChzGeom &g = c->survey;
    ChuArgs A = chz_window<ChuArgs>(c, g, p);
    A.F = g.tile;
    A.nsel = c->K;
    ChusArgs V;
    V.L = c->sv_L;
    V.C = chus_chunk(g, c->sv_L);
    V.M = g.M;
    V.rank = c->sv_rank;
    V.threshold = c->sv_thr;
    auto launch = [&](auto wr) {
        visit_chu_bins(g.M, [&](auto m) {
            visit_chz_fmt(c->fmt, [&](auto fmt) {
                hipLaunchKernelGGL((k_chus<decltype(m)::value, decltype(fmt)::value, decltype(wr)::value>), dim3(chz_grid(g, p->out_count)),
                                   dim3(g.threads), g.lds_bytes, c->stream, A, V, (const ChuPlan *)c->d_uplan, raw, (const float *)c->d_h,
                                   c->d_out[p->buffer].get(), c->d_svpart.get());
            });
        });
    };
    if (write) launch(std::true_type{});
    else launch(std::false_type{});
    hipLaunchKernelGGL(k_chus_finish, dim3((unsigned)(p->out_count / c->sv_L)), dim3(256), 0, c->stream, V, (const float *)c->d_svpart,
                       c->d_svpower.get(), c->d_svfloor.get(), c->d_svmask.get());
}

static void chzr_launch(mfb_channelizer *c, const mfb_channelizer_params *p, const void *raw) {
    const ChzGeom &g = c->plan;
    ChzrArgs R = chz_window<ChzrArgs>(c, g, p);
    R.U = g.U;
    R.Tb = g.Tb;
    R.L = g.L;
    R.S = g.S;
    R.rD = 1.0f / (float)g.D;
    R.tap_stride = c->rtap_stride;
    R.ncplx = c->ncplx;
    R.nreal = c->K - c->ncplx;
    visit_chz_fmt(c->fmt, [&](auto fmt) {
        hipLaunchKernelGGL(k_chzr<decltype(fmt)::value>, dim3(chz_grid(g, p->out_count)), dim3(g.threads), g.lds_bytes, c->stream, R,
                           (const ChzPlan *)c->d_plan, raw, (const float2 *)c->d_rtaps, c->d_out[p->buffer].get());
    });
}

static void chz_launch(mfb_channelizer *c, const mfb_channelizer_params *p, const void *raw) {
    const ChzGeom &g = c->plan;
    ChzArgs A = chz_window<ChzArgs>(c, g, p);
    A.L = g.L;
    A.rD = 1.0f / (float)g.D;
    A.tap_stride = c->max_taps;
    A.ncplx = c->ncplx;
    A.nreal = c->K - c->ncplx;
    visit_chz_fmt(c->fmt, [&](auto fmt) {
        hipLaunchKernelGGL(k_chz<decltype(fmt)::value>, dim3(chz_grid(g, p->out_count)), dim3(g.threads), g.lds_bytes, c->stream, A,
                           (const ChzPlan *)c->d_plan, raw, (const float2 *)c->d_taps, c->d_out[p->buffer].get());
    });
}

// kind: the plan's for a plain call, CHZ_SURVEY for a survey call, which writes the output set only if `write`
static int chz_begin_body(mfb_channelizer *c, const mfb_channelizer_params *p, int kind, bool write = true) {
    HIPCHK(hipSetDevice(c->device));
    const size_t sb = sample_bytes(c->fmt);
    const void *raw = p->device_input;
    if (p->input != MFB_CHZ_INPUT_DEVICE) {
        const int w = p->input == MFB_CHZ_INPUT_PINNED1;
        if (!c->d_in[w]) HIPCHK(c->d_in[w].alloc((size_t)c->max_in * sizeof(float2), hip_malloc));
        HIPCHK(hipMemcpyAsync(c->d_in[w], c->h_in[w], (size_t)p->in_count * sb, hipMemcpyHostToDevice, c->stream));
        raw = c->d_in[w].get();
    }
    c->count[p->buffer] = 0;
    HIPCHK(hipEventRecord(c->t0, c->stream));
    switch (kind) {
        case CHZ_INTEGER: chz_launch(c, p, raw); break;
        case CHZ_RATIONAL: chzr_launch(c, p, raw); break;
        case CHZ_UNIFORM: chu_launch(c, p, raw); break;
        case CHZ_UNIFORM_RATIONAL: chur_launch(c, p, raw); break;
        default: chus_launch(c, p, raw, write); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventRecord(c->done, c->stream));
    c->cur = p->buffer;
    c->count[p->buffer] = write ? p->out_count : 0;    // (0: the set was not written)
    c->nchan[p->buffer] = c->K;
    c->sv_call = kind == CHZ_SURVEY;
    if (c->sv_call) {
        c->sv_wrote = write;
        c->sv_cells = p->out_count / c->sv_L;
    }
    c->busy = true;
    return MFB_OK;
}

// what mfb_channelizer_begin refuses
static int chz_begin_check(mfb_channelizer *c, const mfb_channelizer_params *p) {
    if (!c || !p) return MFB_ERR_ARG;
    if (p->in_count < 1 || p->out_count < 1 || p->in_base < 0 || p->out_base < 0 || (p->buffer != 0 && p->buffer != 1)) return MFB_ERR_ARG;
    if (p->input != MFB_CHZ_INPUT_PINNED0 && p->input != MFB_CHZ_INPUT_PINNED1 && p->input != MFB_CHZ_INPUT_DEVICE) return MFB_ERR_ARG;
    if (p->input == MFB_CHZ_INPUT_DEVICE && !p->device_input) return MFB_ERR_ARG;
    if (p->in_count > CHZ_MAX_IN || p->out_count > CHZ_MAX_OUT || p->in_base >= ((int64_t)1 << 62)) return MFB_ERR_UNSUPPORTED;
    if (p->in_count > c->max_in || p->out_count > c->max_out) return MFB_ERR_ARG;
    if (c->busy) return MFB_ERR_STATE;
    if (!c->have_plan) return MFB_ERR_STATE;
    const int D = c->plan.D;
    if (p->out_base >= (((int64_t)1 << 62) + D - 1) / D) return MFB_ERR_UNSUPPORTED;             // out_base * D < 2^62
    if (p->input == MFB_CHZ_INPUT_DEVICE && ((uintptr_t)p->device_input & (sample_bytes(c->fmt) - 1))) return MFB_ERR_ARG;
    if (p->input != MFB_CHZ_INPUT_DEVICE && !c->h_in[p->input == MFB_CHZ_INPUT_PINNED1]) return MFB_ERR_STATE;
    // every input an output reads, apart from the positions below 0, lies inside the call's input
    int64_t first = 0, last = 0;
    chz_input_span(c->plan, p->out_base, p->out_count, &first, &last);
    if ((first > 0 ? first : 0) < p->in_base || last >= p->in_base + p->in_count) return MFB_ERR_ARG;
    return MFB_OK;
}

extern "C" int mfb_channelizer_begin(mfb_channelizer *c, const mfb_channelizer_params *p) {
    const int rc = chz_begin_check(c, p);
    if (rc) return rc;
    return guarded([&] { return chz_begin_body(c, p, c->plan.kind); });
}

// the output set of the call in flight to the host, on the stream
static hipError_t chz_copy_out(mfb_channelizer *c, float *out_c64) {
    const int b = c->cur;
    const size_t row = (size_t)c->count[b] * sizeof(float2);
    return hipMemcpy2DAsync(out_c64, row, c->d_out[b].get(), (size_t)c->out_stride * sizeof(float2), row, (size_t)c->nchan[b], hipMemcpyDeviceToHost,
                            c->stream);
}

extern "C" int mfb_channelizer_end(mfb_channelizer *c, float *out_c64) {
    if (!c) return MFB_ERR_ARG;
    if (!c->busy || c->sv_call) return MFB_ERR_STATE;          // (a survey call ends with mfb_channelizer_survey_end)
    HIPCHK(hipSetDevice(c->device));
    return c->finish(out_c64 != nullptr, [&] { return chz_copy_out(c, out_c64); });
}

extern "C" int mfb_channelizer_device_output(mfb_channelizer *c, int buffer, int channel, const void **dev_c64, int64_t *nsamples) {
    if (!c || !dev_c64 || (buffer != 0 && buffer != 1) || channel < 0) return MFB_ERR_ARG;
    if (!c->readable(c->busy, buffer) || channel >= c->nchan[buffer]) return MFB_ERR_STATE;
    *dev_c64 = c->d_out[buffer].get() + (size_t)channel * c->out_stride;
    if (nsamples) *nsamples = c->count[buffer];
    return MFB_OK;
}

extern "C" int mfb_channelizer_elapsed_ms(mfb_channelizer *c, float *ms) {
    if (!c || !ms) return MFB_ERR_ARG;
    // ran: a set is written, or the last call was a survey's -- a new plan empties the sets and takes the time with them
    return c->elapsed_ms(*c, c->count[0] || c->count[1] || c->sv_call, ms);
}

// ---- the survey of a uniform plan (channelize_survey_kernels.hpp)
static int chus_set_body(mfb_channelizer *c, int cell_frames, int rank, float threshold) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(chus_drop(c));
    if (!cell_frames) return MFB_OK;
    const ChusTables t = chus_tables(c->survey, cell_frames, c->max_out);
    HIPCHK(c->d_svpart.alloc((size_t)t.chunks * c->M * sizeof(float), hip_malloc));
    HIPCHK(c->d_svpower.alloc((size_t)t.cells * c->M * sizeof(float), hip_malloc));
    HIPCHK(c->d_svfloor.alloc((size_t)t.cells * sizeof(float), hip_malloc));
    HIPCHK(c->d_svmask.alloc((size_t)t.cells * t.words * sizeof(uint32_t), hip_malloc));
    c->sv_rank = rank;
    c->sv_thr = threshold;
    c->sv_L = cell_frames;
    return MFB_OK;
}

extern "C" int mfb_channelizer_set_survey(mfb_channelizer *c, int cell_frames, int rank, float threshold) {
    if (!c) return MFB_ERR_ARG;
    if (!c->M || !c->have_plan || c->busy) return MFB_ERR_STATE;
    if (c->plan.kind == CHZ_UNIFORM_RATIONAL) return MFB_ERR_UNSUPPORTED;      // the survey is a matter of integer plans
    if (cell_frames) {
        if (cell_frames < (1 << CHUS_MIN_LOG2) || cell_frames > (1 << CHUS_MAX_LOG2) || (cell_frames & (cell_frames - 1))) return MFB_ERR_ARG;
        if (rank < 0 || rank >= c->M || !std::isfinite(threshold) || threshold < 1.0f) return MFB_ERR_ARG;
        if (cell_frames > c->max_out) return MFB_ERR_ARG;      // no call of this handle holds one cell
    }
    const int rc = guarded([&] { return chus_set_body(c, cell_frames, rank, threshold); });
    if (rc) (void)chus_drop(c);
    return rc;
}

extern "C" int mfb_channelizer_survey_info(mfb_channelizer *c, int *cell_frames, int *frames_per_workgroup, int *rank, float *threshold) {
    if (!c) return MFB_ERR_ARG;
    if (!c->M || !c->have_plan) return MFB_ERR_STATE;
    if (cell_frames) *cell_frames = c->sv_L;
    if (frames_per_workgroup) *frames_per_workgroup = c->survey.tile;
    if (rank) *rank = c->sv_rank;
    if (threshold) *threshold = c->sv_thr;
    return MFB_OK;
}

extern "C" int mfb_channelizer_survey_begin(mfb_channelizer *c, const mfb_channelizer_params *p, int write_outputs) {
    if (!c || !p) return MFB_ERR_ARG;
    if (!c->M) return MFB_ERR_STATE;
    const int rc = chz_begin_check(c, p);
    if (rc) return rc;
    if (!c->sv_L) return MFB_ERR_STATE;
    if (p->out_base % c->sv_L || p->out_count % c->sv_L) return MFB_ERR_ARG;
    if ((int64_t)c->M * p->out_count > CHU_MAX_SET || (int64_t)c->M * (p->out_count / c->sv_L) > CHUS_MAX_TABLE) return MFB_ERR_UNSUPPORTED;
    return guarded([&] { return chz_begin_body(c, p, CHZ_SURVEY, write_outputs != 0); });
}

extern "C" int mfb_channelizer_survey_end(mfb_channelizer *c, float *out_c64, float *power, float *floor, uint32_t *mask) {
    if (!c) return MFB_ERR_ARG;
    if (!c->busy || !c->sv_call) return MFB_ERR_STATE;         // (a plain call ends with mfb_channelizer_end)
    if (out_c64 && !c->sv_wrote) return MFB_ERR_ARG;           // the call stays in flight
    HIPCHK(hipSetDevice(c->device));
    const size_t cells = (size_t)c->sv_cells;
    return c->finish(out_c64 || power || floor || mask, [&] {
        const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
        hipError_t e = out_c64 ? chz_copy_out(c, out_c64) : hipSuccess;
        if (e == hipSuccess && power) e = hipMemcpyAsync(power, c->d_svpower, cells * c->M * sizeof(float), d2h, c->stream);
        if (e == hipSuccess && floor) e = hipMemcpyAsync(floor, c->d_svfloor, cells * sizeof(float), d2h, c->stream);
        if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c->d_svmask, cells * ((c->M + 31) / 32) * sizeof(uint32_t), d2h, c->stream);
        return e;
    });
}
