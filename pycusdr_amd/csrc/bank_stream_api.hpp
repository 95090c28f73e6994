// bank_stream_api.hpp -- the integer stages behind a batch's symbol decisions (mfb_set_stream_stages; the kernels: stream_kernels.hpp).
// A part of mfbank.hip's one translation unit: included there once, behind bank_clip_api.hpp.  Host code only.
#pragma once

// A14 for the blocks of a batch: one packed launch (search + would-be stash edges + ring) where the templates allow it
static void stream_search_launch(mfb_ctx *c, const StreamArgs &sa, int nb, int Tmax) {
    const size_t words = (size_t)((STREAM_PACK_TAPS + sa.T[0] - 1 + STREAM_EDGE_BACK + sa.nOv + sa.nsym + 31) >> 5) + STREAM_PACK_TAPS / 32 + 4;
    static const bool unpacked = getenv("MFB_STREAM_UNPACKED") != nullptr;       // (A/B switch of tools/chain_kernels.sh)
    if (sa.packed && words * 4 <= 60 * 1024 && !unpacked) {
        hipLaunchKernelGGL(k_stream_search, dim3(nb), dim3(STREAM_SEARCH_THREADS), words * 4, c->stream, sa);
        return;
    }
    hipLaunchKernelGGL(k_stream_sync, dim3(sa.K, nb), dim3(256), (size_t)Tmax + SYNC_SEG + Tmax - 1, c->stream, sa);
    hipLaunchKernelGGL(k_stream_ring, dim3(1), dim3(256), 0, c->stream, sa);
    hipLaunchKernelGGL(k_stream_edges, dim3(nb), dim3(256), 0, c->stream, sa);
}
// the records a launch of the stream stages works on
static void stream_records(StreamArgs &sa, uint8_t *rec0, const RecordLayout &l) {
    sa.rec0 = rec0;
    sa.rec = l.bytes;
    sa.off_sym = l.sym;
    sa.off_cen = l.cen;
    sa.off_mag = l.mag;
    sa.off_bits = l.bits;
    sa.off_cenw = l.cenw;
    sa.off_trust = l.trust;
    sa.off_post = l.post;
    sa.off_end = l.end;
    sa.off_hits = l.hits;
    sa.off_edges = l.edges;
}
// A12 / A13 / A14 of the nb records at rec0 on the device (stream_kernels.hpp), as part 2 of a batch launches them -- and the test seam
// (mfb_debug_stream_stages), by calling this; the state they chain on -- the previous
// batch's tail and bit ring -- sits in carry[parity], this batch leaves its own in carry[1 - parity]
static int stream_stages_enqueue(mfb_ctx *c, uint8_t *rec0, const RecordLayout &l, int nb, int nsym, int parity, const ClipLaunch *tag) {
    StreamArgs sa = c->st;
    stream_records(sa, rec0, l);
    sa.nb = nb;
    sa.nsym = nsym;
    sa.carry_in = c->d_carry[parity];
    sa.carry_out = c->d_carry[1 - parity];
    hipLaunchKernelGGL(k_stream_align, dim3(nb), dim3(STREAM_ALIGN_THREADS), 0, c->stream, sa);
    HIPCHK(hipGetLastError());
    if (tag) {
        // S-band: the clipped-peak tags in the kept trust bytes (DB:830-837), from the flight's own clip indices
        hipLaunchKernelGGL(k_stream_tag, dim3(nb, (nsym + STREAM_TAG_THREADS - 1) / STREAM_TAG_THREADS), dim3(STREAM_TAG_THREADS), 0,
                           c->stream, sa, (const int32_t *)tag->a.idx,
                           (const int32_t *)tag->a.head, CLIP_HEAD);
        HIPCHK(hipGetLastError());
    }
    if (sa.K > 0) {
        int Tmax = 0;
        for (int t = 0; t < sa.K; ++t) Tmax = sa.T[t] > Tmax ? sa.T[t] : Tmax;
        stream_search_launch(c, sa, nb, Tmax);
        HIPCHK(hipGetLastError());
    }
    return MFB_OK;
}

// The integer stages behind the symbol decisions on the device, for batches (stream_kernels.hpp).
extern "C" int mfb_set_stream_stages(mfb_ctx *c, const mfb_stream_params *p) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_and_invalidate(c));
    c->st_on = false;
    if (!p) return MFB_OK;                 // switched off
    // (the LUTs live in the LDS of k_stream_align: 256 rows of a bit LUT, 2048 entries of an NRZ-S LUT -- 2^xcorrMaskSize is 8 ... 32)
    if ((p->lut_mode != 1 && p->lut_mode != 2) || p->lut_rows < 1 || (p->lut_mode == 1 && p->lut_rows > STREAM_LUT8_MAX) ||
        (p->lut_mode == 2 && (p->lut_successors < 1 || (long long)p->lut_rows * 2 * p->lut_successors > STREAM_LUT3_MAX)) || !p->lut || p->overlap_samples < 2 ||
        p->overlap_samples >= c->N || p->overlap_offset < 1 || p->overlap_offset + 1 > STREAM_END_MAX || p->num_templates < 0 ||
        p->num_templates > STREAM_MAX_TMPL || (p->lut_mode == 2 && (p->lut_successors < 1 || p->lut_successors > 64)))
        return MFB_ERR_ARG;
    if (p->num_templates > 0 && (!p->templates || p->bits_overlap < 1 || p->bits_overlap > STREAM_NOV_MAX)) return MFB_ERR_ARG;
    StreamArgs &a = c->st;
    memset(&a, 0, sizeof(a));
    a.N = c->N;
    a.ovw = p->overlap_samples / 2;
    a.o = p->overlap_offset;
    a.thr = p->match_threshold;
    a.err_thr = p->error_threshold;
    a.mode = p->lut_mode;
    a.rows = p->lut_rows;
    a.succ = p->lut_mode == 2 ? p->lut_successors : 0;
    HIPCHK(c->d_lut8.reset());
    HIPCHK(c->d_lut3.reset());
    HIPCHK(c->d_sttmpl.reset());
    if (a.mode == 1) {
        HIPCHK(c->d_lut8.alloc((size_t)a.rows, dev_alloc));
        HIPCHK(hipMemcpy(c->d_lut8, p->lut, (size_t)a.rows, hipMemcpyHostToDevice));
    } else {
        const size_t n = (size_t)a.rows * 2 * a.succ * sizeof(int);
        HIPCHK(c->d_lut3.alloc(n, dev_alloc));
        HIPCHK(hipMemcpy(c->d_lut3, p->lut, n, hipMemcpyHostToDevice));
    }
    a.lut8 = c->d_lut8;
    a.lut3 = c->d_lut3;
    a.K = p->num_templates;
    a.nOv = p->bits_overlap;
    a.max_hits = STREAM_MAX_HITS;
    size_t taps = 0;
    for (int t = 0; t < a.K; ++t) {
        if (p->template_taps[t] < 1 || p->template_taps[t] > 4096) return MFB_ERR_ARG;
        a.T[t] = p->template_taps[t];
        a.thrs[t] = p->template_thresholds[t];
        a.toff[t] = (int)taps;
        taps += (size_t)a.T[t];
    }
    // the packed search (k_stream_search) takes templates of up to STREAM_PACK_TAPS taps in {-1, 0, +1}
    a.packed = a.K > 0;
    memset(a.P, 0, sizeof(a.P));
    memset(a.Q, 0, sizeof(a.Q));
    for (int t = 0; t < a.K && a.packed; ++t) {
        const int8_t *tp = p->templates + a.toff[t];
        if (a.T[t] > STREAM_PACK_TAPS) a.packed = 0;
        for (int q = 0; q < a.T[t] && a.packed; ++q) {
            const int j = a.T[t] - 1 - q;                   // window element the tap multiplies
            if (tp[q] == 1) a.P[t][j >> 5] |= 1u << (j & 31);
            else if (tp[q] == -1) a.Q[t][j >> 5] |= 1u << (j & 31);
            else if (tp[q] != 0) a.packed = 0;
        }
    }
    if (taps) {
        HIPCHK(c->d_sttmpl.alloc(taps, dev_alloc));
        HIPCHK(hipMemcpy(c->d_sttmpl, p->templates, taps, hipMemcpyHostToDevice));
    }
    a.tmpls = c->d_sttmpl;
    for (int i = 0; i < 2; ++i) {
        if (!c->d_carry[i]) HIPCHK(c->d_carry[i].alloc(sizeof(StreamCarry), dev_alloc));
        HIPCHK(hipMemset(c->d_carry[i], 0, sizeof(StreamCarry)));       // valid = 0: nothing known until mfb_stream_seed
    }
    if (!c->h_seed) HIPCHK(c->h_seed.alloc(sizeof(StreamCarry), hip_host_malloc));
    c->carry_cur = 0;
    c->st_on = true;
    return MFB_OK;
}

extern "C" int mfb_stream_seed(mfb_ctx *c, const uint8_t *post, int npost, const uint8_t *end, int nend, const uint8_t *ring, int ring_len) {
    if (!c || npost < 0 || nend < 0 || ring_len < 0 || (npost && !post) || (nend && !end) || (ring_len && !ring)) return MFB_ERR_ARG;
    if (!c->st_on) return MFB_ERR_STATE;
    if (npost > STREAM_POST_MAX || nend > STREAM_END_MAX || ring_len > STREAM_NOV_MAX) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));          // h_seed may still be on its way from the last seed
    StreamCarry *h = c->h_seed;
    memset(h, 0, sizeof(*h));
    h->valid = 1;
    h->npost = npost;
    h->nend = nend;
    if (npost) memcpy(h->post, post, (size_t)npost);
    if (nend) memcpy(h->end, end, (size_t)nend);
    h->ring_valid = ring_len > 0 && ring_len == c->st.nOv;
    h->ring_len = ring_len;
    if (ring_len) memcpy(h->ring, ring, (size_t)ring_len);
    HIPCHK(hipMemcpyAsync(c->d_carry[c->carry_cur], h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
    return MFB_OK;
}
