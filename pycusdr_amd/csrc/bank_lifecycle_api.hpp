// bank_lifecycle_api.hpp -- a bank from mfb_create to mfb_destroy: twiddles, tuning, the kernels' attributes (visit_seg*), streams, timers.
// A part of mfbank.hip's one translation unit: included there once, behind bank_ctx.hpp.  Host code only.
#pragma once

static void make_twiddles(std::vector<cf> &v, int count, double denom, double stepmul) {
    v.resize(count);
    for (int i = 0; i < count; ++i) {
        const double ang = 2.0 * M_PI * (double)i * stepmul / denom;
        v[i] = (cf){(float)cos(ang), (float)sin(ang)};
    }
}

// (cos, tan) pairs of the fused-twiddle transforms (fft_core.hpp, MFB_FFT_FUSED), appended to the W_L table: angle 2 pi u / L.
// An angle of exactly pi/2 (one lane of stage 1) becomes (2^-40, 2^40): c t = 1 exactly, and c b vanishes in the rounding of the sum.
static cf ct_pair(long u, int L) {
    const double ang = 2.0 * M_PI * (double)u / (double)L;
    double c = cos(ang);
    const double s = sin(ang);
    if (fabs(c) < 1e-9) c = 0x1p-40;
    return (cf){(float)c, (float)(s / c)};
}
static void append_fused_tables(std::vector<cf> &v, int L) {
    if (L == 256) {            // F256Regs: [16 lanes][8]
        for (int g = 0; g < 16; ++g) {
            const long u[8] = {8 * g, 4 * g, 2 * g, 2 * g + 32, g, g + 16, g + 32, g + 48};
            for (int k = 0; k < 8; ++k) v.push_back(ct_pair(u[k], L));
        }
    } else if (L == 2048) {    // F2048Regs: [64 positions][16], then W_64^p, p < 32
        for (int g = 0; g < 64; ++g) {
            v.push_back(ct_pair(16 * g, L));
            v.push_back(ct_pair(8 * g, L));
            for (int q = 0; q < 2; ++q) v.push_back(ct_pair(4 * g + 256 * q, L));
            for (int q = 0; q < 4; ++q) v.push_back(ct_pair(2 * g + 128 * q, L));
            for (int q = 0; q < 8; ++q) v.push_back(ct_pair(g + 64 * q, L));
        }
        for (int p = 0; p < 32; ++p) v.push_back(ct_pair(32 * p, L));
    }
}

static int upload_tw(DevBuf<cf> *dst, const std::vector<cf> &v) {
    HIPCHK(dst->alloc(v.size() * sizeof(cf), dev_alloc));
    HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(cf), hipMemcpyHostToDevice));
    return MFB_OK;
}

// pass-2 work split: sub-rows (n1 values) per workgroup; a power of two in [RB, N1]
static void set_rows_per_block(mfb_ctx *c, int srb) {
    const int NT = c->N2 / 16;
    const int RB = NT >= 256 ? 1 : 256 / NT;
    int p = 1;
    while (p * 2 <= srb) p *= 2;
    srb = p;
    if (srb < RB) srb = RB;
    if (srb > c->N1) srb = c->N1;
    c->srb = srb;
    c->parts = c->N1 / srb;
}

static int default_chunk(const mfb_ctx *c) {
    const size_t row_bytes = (size_t)c->N * sizeof(cf) * c->MU;
    size_t ch = ((size_t)8 << 30) / row_bytes;
    if (ch < 1) ch = 1;
    if (ch > (size_t)c->Dtot) ch = c->Dtot;
    if (ch * c->MU > 65535) ch = 65535 / c->MU;
    return (int)ch;
}

// ---- per-device kernel attributes ------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): it is set for every
// instantiation that can need more than 48 KiB whenever a handle is created, on that handle's device.
template <int L1>
static int attr_p1() {
    if (P1Cfg<L1>::lds_bytes > 48 * 1024) {
        const int b = (int)P1Cfg<L1>::lds_bytes;
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_BANK>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_FWDC>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_FWDR>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
    }
    return MFB_OK;
}
template <int L2>
static int attr_p2() {
    if (P2Cfg<L2>::lds_bytes > 48 * 1024) {
        const int b = (int)P2Cfg<L2>::lds_bytes;
        HIPCHK(hipFuncSetAttribute((const void *)k_pass2<L2, MODE_REDUCE>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass2<L2, MODE_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
    }
    return MFB_OK;
}
// ---- the search's kernel instantiations, enumerated ONCE per family ----------------------------------------------------------------
// visit_*(f) calls f(tag) for every instantiation of the family until a call returns something other than VISIT_NEXT, and returns
// that.  Setting the attributes visits all of a family; a launch visits until (segment length, mode or variant, pv) matches.  The
// ranges are seg_ppl, segf_has_sumq and segf_has_presum themselves, and nothing else is instantiated: no launch reaches a kernel whose
// attribute was never set.  PV: valid register slots of a complete segment (half ... all) for the branch-free form, -1 = masked.
constexpr int VISIT_NEXT = -1;
template <int SEGL_, int MODE_, int PV_>
struct SegInst {       // k_seg<L, MODE, PV> | k_segf<L, PV, SUMQ = MODE>
    static constexpr int SEGL = SEGL_, L = 1 << SEGL_, MODE = MODE_, PV = PV_;
};
template <int SEGL, class F, int... I>
static int visit_seg_l(F &f, std::integer_sequence<int, I...>) {
    int rc = f(SegInst<SEGL, SEG_STORE, -1>{});
    if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, SEG_REDUCE, -1>{});
    (void)((rc == VISIT_NEXT && (rc = f(SegInst<SEGL, SEG_REDUCE, seg_ppl(1 << SEGL) / 2 + I>{})) == VISIT_NEXT) && ...);
    return rc;
}
using SegLens = std::integer_sequence<int, 8, 9, 10, 11, 12, SEG_LOG2L_MAX>;
template <class F, int... SEGL>
static int visit_seg(F f, std::integer_sequence<int, SEGL...>) {
    int rc = VISIT_NEXT;
    (void)(((rc = visit_seg_l<SEGL>(f, SegSlots<(1 << SEGL)>{})) == VISIT_NEXT) && ...);
    return rc;
}
template <int SEGL, class F, int... I>
static int visit_segf_l(F &f, std::integer_sequence<int, I...>) {
    int rc = VISIT_NEXT;
    auto variants = [&](auto pv) {
        constexpr int L = 1 << SEGL, PV = decltype(pv)::value;
        rc = f(SegInst<SEGL, 0, PV>{});
        if constexpr (segf_has_sumq<L, PV>())
            if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, 1, PV>{});
        if constexpr (segf_has_presum<L, PV>())
            if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, 2, PV>{});
        return rc == VISIT_NEXT;
    };
    (void)(variants(std::integral_constant<int, seg_ppl(1 << SEGL) / 2 + I>{}) && ...);
    return rc;
}
template <class F>
static int visit_segf(F f) {
    const int rc = visit_segf_l<8>(f, SegSlots<256>{});
    return rc != VISIT_NEXT ? rc : visit_segf_l<11>(f, SegSlots<2048>{});
}
#define MFB_MAX_LDS(K_, B_) HIPCHK(hipFuncSetAttribute((const void *)K_, hipFuncAttributeMaxDynamicSharedMemorySize, B_))
static int set_kernel_attributes(const mfb_ctx *c) {
    int rc = MFB_OK;
    switch (c->l1) {
        case 5: rc = attr_p1<32>(); break;
        case 6: rc = attr_p1<64>(); break;
        case 7: rc = attr_p1<128>(); break;
        case 8: rc = attr_p1<256>(); break;
        case 9: rc = attr_p1<512>(); break;
    }
    if (rc) return rc;
    switch (c->l2) {
        case 13: rc = attr_p2<8192>(); break;
        default: break;   // <= 4096 points: 35 KiB
    }
    if (rc) return rc;
    rc = visit_seg([](auto k) -> int {
        using K = decltype(k);
        MFB_MAX_LDS((k_seg<K::L, K::MODE, K::PV>), seg_lds_bytes(K::SEGL, SEG_REDUCE, seg_mpb_cap(K::SEGL)));
        return VISIT_NEXT;
    }, SegLens{});
    if (rc == VISIT_NEXT)
        rc = visit_segf([](auto k) -> int {
            using K = decltype(k);
            MFB_MAX_LDS((k_segf<K::L, K::PV, K::MODE>), segf_lds_bytes<K::L>(segf_rows_cap(K::L)));
            return VISIT_NEXT;
        });
    if (rc != VISIT_NEXT) return rc;
    MFB_MAX_LDS((k_segw<SEGW_PV, SEGW_KT>), segw_lds_bytes());
    return MFB_OK;
}
#undef MFB_MAX_LDS

static int create_impl(mfb_ctx *c) {
    HIPCHK(hipStreamCreateWithFlags(out(c->own_stream), hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIPCHK(hipEventCreate(out(c->t0)));
    HIPCHK(hipEventCreate(out(c->t1)));
    int rc = set_kernel_attributes(c);
    if (rc) return rc;
    const int M = c->M;
    const size_t nb = (size_t)c->N * sizeof(cf);
    HIPCHK(c->h_in.alloc(nb, hip_host_malloc));
    memset(c->h_in, 0, nb);
    // three arrays of at most N/2 symbol decisions, the block scalars and the two SNR windows of mfb_receive_block
    c->back_cap = (size_t)3 * (c->N / 2) * sizeof(int) + ((size_t)256 << 10);
    if (c->back_cap < ((size_t)64 << 10)) c->back_cap = (size_t)64 << 10;
    HIPCHK(c->h_back.alloc(c->back_cap, hip_host_malloc));
    HIPCHK(c->h_pick.alloc(4 * sizeof(uint32_t), hip_host_malloc_coherent));
    memset(c->h_pick, 0, 4 * sizeof(uint32_t));          // pick 0 is never asked for
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_pick_dev, c->h_pick, 0));
    HIPCHK(c->d_x.alloc(nb, dev_alloc));
    HIPCHK(c->d_X.alloc(nb, dev_alloc));
    HIPCHK(c->d_masks.alloc(nb * M, dev_alloc));
    HIPCHK(c->d_xc.alloc(nb * M, dev_alloc));
    HIPCHK(c->d_P.alloc(nb, dev_alloc));
    HIPCHK(c->d_env.alloc((size_t)c->N * sizeof(float), dev_alloc));
    HIPCHK(c->d_shifts.alloc((size_t)c->Dtot * sizeof(int), dev_alloc));
    if ((rc = reserve_partials(c, (size_t)c->Dtot * M * c->N1))) return rc;
    HIPCHK(c->d_sum.alloc((size_t)c->Dtot * M * sizeof(float), dev_alloc));
    HIPCHK(hipMemset(c->d_sum, 0, (size_t)c->Dtot * M * sizeof(float)));
    HIPCHK(c->d_res.alloc(2 * sizeof(float), dev_alloc));
    HIPCHK(c->d_uniq.alloc((size_t)M * sizeof(int), dev_alloc));
    HIPCHK(c->d_rep.alloc((size_t)M * sizeof(int), dev_alloc));
    HIPCHK(c->d_cr.alloc(3 * sizeof(float), dev_alloc));
    c->cap = c->N / 2;  // symbols never shorter than 2 samples
    HIPCHK(c->d_sym.alloc((size_t)c->cap * sizeof(int), dev_alloc));
    HIPCHK(c->d_cen.alloc((size_t)c->cap * sizeof(int), dev_alloc));
    HIPCHK(c->d_mag.alloc((size_t)c->cap * sizeof(float), dev_alloc));
    // one row for the plain forward transforms; the search's share is sized when the filters arrive
    if ((rc = alloc_Z(c))) return rc;
    // block path (mfb_receive_block*): everything it needs exists before the first block -- page-locking memory and creating
    // events inside a stream of blocks costs milliseconds
    if ((rc = blkout_reserve(c, 1024))) return rc;
    for (int i = 0; i < 2; ++i) {
        // scalars + three arrays of the symbols a rate window of +-10 % around 4 samples per symbol admits + the two windows
        c->blk_cap[i] = rec_layout(c->band_cap, c->N / 3).bytes;
        HIPCHK(c->h_blk[i].alloc(c->blk_cap[i], hip_host_malloc));
        HIPCHK(hipEventCreateWithFlags(out(c->ev_blk[i]), hipEventDisableTiming));
    }

    std::vector<cf> t;
    make_twiddles(t, c->N1, (double)c->N1, 1.0);
    if ((rc = upload_tw(&c->d_tw1, t))) return rc;
    make_twiddles(t, c->N2, (double)c->N2, 1.0);
    if ((rc = upload_tw(&c->d_tw2, t))) return rc;
    make_twiddles(t, 1 << c->lo, (double)c->N, 1.0);
    if ((rc = upload_tw(&c->d_twLo, t))) return rc;
    make_twiddles(t, c->N >> c->lo, (double)c->N, (double)(1 << c->lo));
    if ((rc = upload_tw(&c->d_twHi, t))) return rc;
    c->d_in = c->d_x;
    return MFB_OK;
}

struct CtxDestroy {
    void operator()(mfb_ctx *c) const { (void)mfb_destroy(c); }
};
static int create_body(mfb_ctx **out, int device, int log2N, int num_dopplers, int doppler_offset, int M,
                       int window_width, int sum_all_masks, int code_search_mask_offset) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (num_dopplers < 1 || doppler_offset < 0 || M < 1 || M > 64 || window_width < 1 || (window_width & 1) == 0 ||
        code_search_mask_offset < 0 || 2 * code_search_mask_offset >= M)
        return MFB_ERR_ARG;
    if (log2N < 10 || log2N > 22) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));

    // any failure below -- a status or an exception -- frees what was allocated so far (mfb_destroy tolerates partial handles):
    // the counterpart of the reference's context teardown, demodulator_base.py:517-530
    std::unique_ptr<mfb_ctx, CtxDestroy> c(new mfb_ctx());
    c->device = device;
    c->num_cus = ncu > 0 ? ncu : 256;
    c->log2N = log2N;
    c->N = 1 << log2N;
    // N = N1 * N2: columns of at most 256 points, rows of at most 8192 (2^22 = 512 x 8192: a 16384-point row would
    // need 1024 threads at 128 VGPRs and spilled > 100 registers)
    c->l1 = log2N / 2 < 8 ? log2N / 2 : 8;
    if (log2N - c->l1 > 13) c->l1 = log2N - 13;
    c->l2 = log2N - c->l1;
    c->N1 = 1 << c->l1;
    c->N2 = 1 << c->l2;
    c->lo = (log2N + 1) / 2;
    c->D = num_dopplers;
    c->Doff = doppler_offset;
    c->Dtot = num_dopplers + doppler_offset;
    c->M = M;
    c->W = window_width;
    c->sum_all = sum_all_masks ? 1 : 0;
    c->cs_off = code_search_mask_offset;
    // Two-pass search, Doppler bins per launch: as many as an 8 GiB intermediate holds.  Measured on
    // MI355X (C2: D=256, M=8, N=2^20): long persistent loops amortise the per-workgroup twiddle setup
    // and keep each XCD's L2 serving the filter tile to many Doppler streams, so big chunks win (chunk
    // 16: 9.8 ms, 64: 6.65 ms, 128: 6.55 ms per block) -- but a 16 GiB intermediate (chunk 256) costs
    // 0.4 ms more than two 8 GiB launches.  Keeping the intermediate inside the 256 MiB Infinity
    // Cache (chunk 1-2) does not pay: the cache streams no faster than HBM (tools/ubench/mall.hip).
    c->MU = M;
    c->chunk_auto = true;
    c->chunk = default_chunk(c.get());
    c->mpb = M < 8 ? M : 8;
    c->jsplit = 32;
    set_rows_per_block(c.get(), 64);
    c->path_req = MFB_PATH_AUTO;
    c->path = MFB_PATH_TWOPASS;
    if ((rc = create_impl(c.get()))) return rc;
    *out = c.release();
    return MFB_OK;
}
extern "C" int mfb_create(mfb_ctx **out, int device, int log2N, int num_dopplers, int doppler_offset, int M,
                          int window_width, int sum_all_masks, int code_search_mask_offset) {
    return guarded([&] { return create_body(out, device, log2N, num_dopplers, doppler_offset, M, window_width, sum_all_masks, code_search_mask_offset); });
}

extern "C" int mfb_destroy(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->s2) (void)hipStreamSynchronize(c->s2);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->in_stream) (void)hipStreamSynchronize(c->in_stream);
    for_each_graph(c, -1, graph_drop);
    delete c;       // ~mfb_ctx: every buffer and event, then the streams (see the struct)
    return MFB_OK;
}

extern "C" int mfb_set_stream(mfb_ctx *c, void *s) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_and_invalidate(c));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return MFB_OK;
}

// A share of the device's compute units for this handle's launches (include/mfbank.h): the handle's own stream is replaced by one
// created with a CU mask -- compute unit i belongs to part i % parts.
extern "C" int mfb_set_cu_share(mfb_ctx *c, int part, int parts) {
    if (!c || parts < 1 || parts > 16 || part < 0 || part >= parts) return MFB_ERR_ARG;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    Stream fresh;
    if (parts == 1) {
        HIPCHK(hipStreamCreateWithFlags(out(fresh), hipStreamNonBlocking));
    } else {
        const int words = (c->num_cus + 31) / 32;
        std::vector<uint32_t> mask((size_t)words, 0u);
        int mine = 0;
        for (int i = 0; i < c->num_cus; ++i)
            if (i % parts == part) {
                mask[(size_t)i / 32] |= 1u << (i % 32);
                ++mine;
            }
        if (!mine) return MFB_ERR_ARG;
        HIPCHK(hipExtStreamCreateWithCUMask(out(fresh), (uint32_t)words, mask.data()));
    }
    const bool was_own = c->stream == c->own_stream;
    std::swap(c->own_stream, fresh);
    if (was_own) c->stream = c->own_stream;
    c->cu_part = part;
    c->cu_parts = parts;
    ++c->epoch;
    HIPCHK(fresh.reset());        // (the old one; the handle is whole whatever this says)
    return MFB_OK;
}

extern "C" int mfb_set_tuning(mfb_ctx *c, int chunk, int mpb, int rows_per_block, int jsplit) {
    if (!c || chunk < 0 || mpb < 0 || rows_per_block < 0 || jsplit < 0) return MFB_ERR_ARG;
    ++c->epoch;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    if (rows_per_block > 0) set_rows_per_block(c, rows_per_block);
    if (jsplit > 0) c->jsplit = jsplit;
    if (chunk > 0) {
        c->chunk = chunk > c->Dtot ? c->Dtot : chunk;
        c->chunk_auto = false;
    }
    if (c->chunk * c->MU > 65535) c->chunk = 65535 / c->MU;  // grid.y limit of pass 2
    if (mpb > 0) c->mpb = mpb > c->M ? c->M : mpb;
    if (!c->have_filters) return MFB_OK;   // the intermediate is sized when the filters arrive
    return alloc_Z(c);
}
extern "C" int mfb_get_tuning(mfb_ctx *c, int *chunk, int *mpb, int *rows_per_block, int *jsplit) {
    if (!c) return MFB_ERR_ARG;
    if (chunk) *chunk = c->chunk;
    if (mpb) *mpb = c->mpb;
    if (rows_per_block) *rows_per_block = c->srb;
    if (jsplit) *jsplit = c->jsplit;
    return MFB_OK;
}

extern "C" int mfb_get_info(mfb_ctx *c, int *N1, int *N2, int *unique_filters) {
    if (!c) return MFB_ERR_ARG;
    if (N1) *N1 = c->N1;
    if (N2) *N2 = c->N2;
    if (unique_filters) *unique_filters = c->MU;
    return MFB_OK;
}

extern "C" int mfb_timer_start(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return MFB_OK;
}
extern "C" int mfb_timer_stop(mfb_ctx *c, float *ms) {
    if (!c || !ms) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    HIPCHK(hipEventElapsedTime(ms, c->t0, c->t1));
    return MFB_OK;
}
extern "C" int mfb_profile_enable(mfb_ctx *c, int on) {
    if (!c) return MFB_ERR_ARG;
    c->prof = on != 0;
    return MFB_OK;
}
extern "C" int mfb_profile_read(mfb_ctx *c, int counts[2], float total_ms[2]) {
    if (!c || !counts || !total_ms) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    for (int w = 0; w < 2; ++w) {
        counts[w] = (int)(c->ev[w].size() / 2);
        double tot = 0.0;
        for (size_t i = 0; i + 1 < c->ev[w].size(); i += 2) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, c->ev[w][i], c->ev[w][i + 1]));
            tot += ms;
        }
        total_ms[w] = (float)tot;
        for (auto &e : c->ev[w]) c->ev_pool.push_back(std::move(e));
        c->ev[w].clear();
    }
    return MFB_OK;
}
extern "C" int mfb_sync(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    return MFB_OK;
}
