// sync_api.hpp -- the host side of the sync correlator: the handle-less calls and their workspaces, the sync finder, the packed form.
// A part of mfbank.hip's one translation unit: included there once, behind sync_kernels.hpp and stage_handle.hpp.  Host code only.
#pragma once

// Workspaces of the (handle-less) sync correlator.  Every call borrows a workspace -- device buffers
// that only grow, plus a stream of its own -- from a per-device pool and returns it afterwards, so
// concurrent callers (two decoder threads, two demodulator instances on one device) never share
// buffers or serialise on the null stream.  The pool itself is guarded by a mutex.
struct SyncWs {
    Stream stream;            // (first: it goes last)
    DevBuf<uint8_t> bits;
    DevBuf<int8_t> tmpl;
    DevBuf<int32_t> out;
    DevBuf<int> seg;        // segcnt | segoff | counts
    DevBuf<int32_t> hits;   // hit_idx | hit_score
    size_t cap_bits = 0, cap_tmpl = 0, cap_out = 0, cap_seg = 0, cap_hits = 0;
    // small calls (one block's bit stream, a few templates): inputs and results each travel as ONE packed copy
    // through page-locked staging -- every separate copy of pageable memory costs a round trip of its own
    HostBuf<uint8_t> h_stage;
    DevBuf<uint8_t> d_stage;
    size_t cap_hstage = 0, cap_dstage = 0;
};
#define SYNC_STAGE_MAX ((size_t)1 << 20)
static std::mutex g_sync_mu;
static std::vector<SyncWs *> g_sync_pool[SYNC_MAX_DEVICES];

static SyncWs *ws_acquire(int device) {
    {
        std::lock_guard<std::mutex> lk(g_sync_mu);
        auto &pool = g_sync_pool[device];
        if (!pool.empty()) {
            SyncWs *w = pool.back();
            pool.pop_back();
            return w;
        }
    }
    std::unique_ptr<SyncWs> w(new SyncWs());
    // highest priority: the decoder's small searches run while the demodulator's stream has the next block's kernels queued
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(out(w->stream), hipStreamNonBlocking, hi) != hipSuccess) return nullptr;
    return w.release();      // (the pool keeps its workspaces until the process exits)
}
static void ws_release(int device, SyncWs *w) {
    std::lock_guard<std::mutex> lk(g_sync_mu);
    g_sync_pool[device].push_back(w);
}
struct WsLease {   // returns the workspace on every exit path
    int device;
    SyncWs *w;
    ~WsLease() {
        if (w) ws_release(device, w);
    }
};

static int ws_reserve(Mem<DevFree> *p, size_t *cap, size_t need) {
    HIPCHK(reserve(*p, *cap, need, need, hip_malloc));
    return MFB_OK;
}

extern "C" int mfb_sync_correlate(int device, const uint8_t *bits, int B, int L, const int8_t *tmpl, int T, int32_t *scores) {
    if (!bits || !tmpl || !scores || B < 1 || L < 1 || T < 1 || T > 4096) return MFB_ERR_ARG;
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    const int outLen = L + T - 1;
    WsLease lease{device, ws_acquire(device)};
    if (!lease.w) return MFB_ERR_HIP;
    SyncWs &w = *lease.w;
    if ((rc = ws_reserve(&w.bits, &w.cap_bits, (size_t)B * L))) return rc;
    if ((rc = ws_reserve(&w.tmpl, &w.cap_tmpl, (size_t)T))) return rc;
    if ((rc = ws_reserve(&w.out, &w.cap_out, (size_t)B * outLen * sizeof(int32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(w.bits, bits, (size_t)B * L, hipMemcpyHostToDevice, w.stream));
    HIPCHK(hipMemcpyAsync(w.tmpl, tmpl, (size_t)T, hipMemcpyHostToDevice, w.stream));
    const int bs = 256;
    const size_t lds = (size_t)T + bs + T - 1;
    hipLaunchKernelGGL(k_sync_corr, dim3((outLen + bs - 1) / bs, B), dim3(bs), lds, w.stream, w.bits, w.tmpl, w.out, L, T);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores, w.out, (size_t)B * outLen * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
    HIPCHK(hipStreamSynchronize(w.stream));
    return MFB_OK;
}


// K templates against the same B bit streams; template t: T[t] taps at tmpls + sum(T[0..t)), threshold thr[t];
// its results sit at counts + t*B, hit_idx / hit_score + t*B*max_hits.
static int sync_find_impl(int device, const uint8_t *bits, int B, int L, const int8_t *tmpls, const int *T, const int *thr, int K,
                          int max_hits, int32_t *hit_idx, int32_t *hit_score, int32_t *counts) {
    if (!bits || !tmpls || !T || !thr || !hit_idx || !hit_score || !counts || B < 1 || L < 1 || K < 1 || K > 16 || max_hits < 1)
        return MFB_ERR_ARG;
    size_t taps = 0;
    int Tmax = 0;
    for (int t = 0; t < K; ++t) {
        if (T[t] < 1 || T[t] > 4096) return MFB_ERR_ARG;
        taps += (size_t)T[t];
        if (T[t] > Tmax) Tmax = T[t];
    }
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    const int nseg = (L + Tmax - 1 + SYNC_SEG - 1) / SYNC_SEG;      // segments of the longest output
    WsLease lease{device, ws_acquire(device)};
    if (!lease.w) return MFB_ERR_HIP;
    SyncWs &w = *lease.w;
    const size_t nbits = (size_t)B * L;
    const size_t res_ints = (size_t)K * B * (1 + 2 * (size_t)max_hits);       // counts | idx | score, template-major
    const bool packed = align16(taps) + nbits <= SYNC_STAGE_MAX && res_ints * sizeof(int32_t) <= SYNC_STAGE_MAX;
    if ((rc = ws_reserve(&w.seg, &w.cap_seg, ((size_t)2 * B * nseg) * sizeof(int)))) return rc;
    if ((rc = ws_reserve(&w.hits, &w.cap_hits, res_ints * sizeof(int32_t)))) return rc;
    int32_t *d_counts = w.hits, *d_idx = w.hits + (size_t)K * B, *d_sc = d_idx + (size_t)K * B * max_hits;
    const uint8_t *d_bits;
    const int8_t *d_tmpl;
    if (packed) {
        const size_t in_bytes = align16(taps) + nbits;
        const size_t hneed = in_bytes > res_ints * sizeof(int32_t) ? in_bytes : res_ints * sizeof(int32_t);
        HIPCHK(reserve(w.h_stage, w.cap_hstage, hneed, hneed, hip_host_malloc));
        if ((rc = ws_reserve(&w.d_stage, &w.cap_dstage, in_bytes))) return rc;
        memcpy(w.h_stage, tmpls, taps);
        memcpy(w.h_stage + align16(taps), bits, nbits);
        HIPCHK(hipMemcpyAsync(w.d_stage, w.h_stage, in_bytes, hipMemcpyHostToDevice, w.stream));
        d_tmpl = (const int8_t *)w.d_stage.get();
        d_bits = w.d_stage + align16(taps);
    } else {
        if ((rc = ws_reserve(&w.bits, &w.cap_bits, nbits))) return rc;
        if ((rc = ws_reserve(&w.tmpl, &w.cap_tmpl, taps))) return rc;
        HIPCHK(hipMemcpyAsync(w.bits, bits, nbits, hipMemcpyHostToDevice, w.stream));
        HIPCHK(hipMemcpyAsync(w.tmpl, tmpls, taps, hipMemcpyHostToDevice, w.stream));
        d_bits = w.bits;
        d_tmpl = w.tmpl;
    }
    int *segcnt = w.seg, *segoff = w.seg + (size_t)B * nseg;
    size_t toff = 0;
    if ((long long)B * nseg * K <= 64) {
        // the decoder's case: everything in one launch (k_sync_small)
        SyncSmallArgs sa;
        size_t o = 0;
        for (int t = 0; t < K; ++t) {
            sa.T[t] = T[t];
            sa.thr[t] = thr[t];
            sa.toff[t] = (int)o;
            o += (size_t)T[t];
        }
        const size_t lds = (size_t)Tmax + SYNC_SEG + Tmax - 1;
        hipLaunchKernelGGL(k_sync_small, dim3(K, B), dim3(256), lds, w.stream, d_bits, d_tmpl, sa, B, L, max_hits, d_counts, d_idx, d_sc);
        HIPCHK(hipGetLastError());
    } else
    for (int t = 0; t < K; ++t) {
        const int Tt = T[t];
        const int ns = (L + Tt - 1 + SYNC_SEG - 1) / SYNC_SEG;
        const size_t lds = (size_t)Tt + SYNC_SEG + Tt - 1;
        int32_t *ci = d_counts + (size_t)t * B, *ii = d_idx + (size_t)t * B * max_hits, *si = d_sc + (size_t)t * B * max_hits;
        hipLaunchKernelGGL((k_sync_find<false>), dim3(ns, B), dim3(256), lds, w.stream, d_bits, d_tmpl + toff, L, Tt, thr[t], ns, segcnt,
                           (const int *)nullptr, max_hits, (int32_t *)nullptr, (int32_t *)nullptr);
        hipLaunchKernelGGL(k_sync_scan, dim3((B + 63) / 64), dim3(64), 0, w.stream, (const int *)segcnt, segoff, ci, B, ns);
        hipLaunchKernelGGL((k_sync_find<true>), dim3(ns, B), dim3(256), lds, w.stream, d_bits, d_tmpl + toff, L, Tt, thr[t], ns, segcnt,
                           (const int *)segoff, max_hits, ii, si);
        HIPCHK(hipGetLastError());
        toff += (size_t)Tt;
    }
    const size_t nc = (size_t)K * B, nh = (size_t)K * B * max_hits;
    if (packed) {
        HIPCHK(hipMemcpyAsync(w.h_stage, w.hits, res_ints * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipStreamSynchronize(w.stream));
        const int32_t *r = (const int32_t *)w.h_stage.get();
        memcpy(counts, r, nc * sizeof(int32_t));
        memcpy(hit_idx, r + nc, nh * sizeof(int32_t));
        memcpy(hit_score, r + nc + nh, nh * sizeof(int32_t));
    } else {
        HIPCHK(hipMemcpyAsync(counts, d_counts, nc * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipMemcpyAsync(hit_idx, d_idx, nh * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipMemcpyAsync(hit_score, d_sc, nh * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipStreamSynchronize(w.stream));
    }
    return MFB_OK;
}

extern "C" int mfb_sync_find(int device, const uint8_t *bits, int B, int L, const int8_t *tmpl, int T, int threshold,
                             int max_hits, int32_t *hit_idx, int32_t *hit_score, int32_t *counts) {
    return sync_find_impl(device, bits, B, L, tmpl, &T, &threshold, 1, max_hits, hit_idx, hit_score, counts);
}

extern "C" int mfb_sync_find_multi(int device, const uint8_t *bits, int B, int L, const int8_t *tmpls, const int *T,
                                   const int *thresholds, int ntmpl, int max_hits, int32_t *hit_idx, int32_t *hit_score,
                                   int32_t *counts) {
    return sync_find_impl(device, bits, B, L, tmpls, T, thresholds, ntmpl, max_hits, hit_idx, hit_score, counts);
}

// ---- a decoder's own sync finder -------------------------------------------------------------------------------------------
// The decoder searches the SAME templates in every block's bit stream (DEC:96-113).  A finder object keeps them on the
// device together with a stream, page-locked staging and result buffers of its own, and splits the search into begin
// (copy in, enqueue, return) and end (wait, copy out): the caller overlaps the round trip with its other work.
struct mfb_syncfinder : StageHandle {
    int K = 0, max_hits = 0, Tmax = 0;
    std::vector<int> T, thr;
    DevBuf<int8_t> d_tmpl;
    DevBuf<uint8_t> d_bits;
    HostBuf<uint8_t> h_bits;
    int cap_bits = 0;
    DevBuf<int32_t> d_res;         // counts[K] | idx[K][max_hits] | score[K][max_hits]
    HostBuf<int32_t> h_res;
    DevBuf<int> d_seg;             // segcnt | segoff of the multi-pass form (long streams)
    size_t cap_seg = 0;
    SyncSmallArgs sa = {};
};

// fn: dev_alloc at create, hip_malloc when a longer stream makes the buffers grow
static int sf_reserve_bits(mfb_syncfinder *f, int L, AllocFn fn) {
    if (L <= f->cap_bits) return MFB_OK;
    HIPCHK(hipStreamSynchronize(f->stream));
    f->cap_bits = 0;
    const int cap = L + L / 2 + 1024;
    HIPCHK(f->d_bits.alloc((size_t)cap, fn));
    HIPCHK(f->h_bits.alloc((size_t)cap, hip_host_malloc));
    f->cap_bits = cap;
    return MFB_OK;
}

extern "C" int mfb_syncfinder_destroy(mfb_syncfinder *f) { return stage_destroy(f); }

static int sf_create_impl(mfb_syncfinder *f, const int8_t *tmpls, int max_bits) {
    size_t taps = 0;
    for (int t = 0; t < f->K; ++t) {
        f->sa.T[t] = f->T[t];
        f->sa.thr[t] = f->thr[t];
        f->sa.toff[t] = (int)taps;
        taps += (size_t)f->T[t];
    }
    HIPCHK(f->d_tmpl.alloc(taps, dev_alloc));
    HIPCHK(hipMemcpy(f->d_tmpl, tmpls, taps, hipMemcpyHostToDevice));
    const size_t res_bytes = (size_t)f->K * (1 + 2 * (size_t)f->max_hits) * sizeof(int32_t);
    HIPCHK(f->d_res.alloc(res_bytes, dev_alloc));
    HIPCHK(f->h_res.alloc(res_bytes, hip_host_malloc));
    return sf_reserve_bits(f, max_bits, dev_alloc);
}

extern "C" int mfb_syncfinder_create(mfb_syncfinder **out, int device, const int8_t *tmpls, const int *T, const int *thresholds, int ntmpl,
                                     int max_bits, int max_hits) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (!tmpls || !T || !thresholds || ntmpl < 1 || ntmpl > 16 || max_bits < 1 || max_hits < 1) return MFB_ERR_ARG;
    for (int t = 0; t < ntmpl; ++t)
        if (T[t] < 1 || T[t] > 4096) return MFB_ERR_ARG;
    return stage_create(out, device, [&](mfb_syncfinder *f) {
        f->K = ntmpl;
        f->max_hits = max_hits;
        f->T.assign(T, T + ntmpl);
        f->thr.assign(thresholds, thresholds + ntmpl);
        f->Tmax = 0;
        for (int t = 0; t < ntmpl; ++t) f->Tmax = T[t] > f->Tmax ? T[t] : f->Tmax;
        return sf_create_impl(f, tmpls, max_bits);
    }, true);      // (a stream of the highest priority, as the handle-less calls' workspaces have)
}

extern "C" int mfb_syncfinder_begin(mfb_syncfinder *f, const uint8_t *bits, int L) {
    if (!f || !bits || L < 1) return MFB_ERR_ARG;
    if (f->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(f->device));
    int rc = sf_reserve_bits(f, L, hip_malloc);
    if (rc) return rc;
    memcpy(f->h_bits, bits, (size_t)L);
    HIPCHK(hipMemcpyAsync(f->d_bits, f->h_bits, (size_t)L, hipMemcpyHostToDevice, f->stream));
    const int K = f->K, mh = f->max_hits;
    int32_t *d_counts = f->d_res, *d_idx = f->d_res + K, *d_sc = d_idx + (size_t)K * mh;
    const int nseg = (L + f->Tmax - 1 + SYNC_SEG - 1) / SYNC_SEG;
    if (nseg <= 16) {
        const size_t lds = (size_t)f->Tmax + SYNC_SEG + f->Tmax - 1;
        hipLaunchKernelGGL(k_sync_small, dim3(K, 1), dim3(256), lds, f->stream, (const uint8_t *)f->d_bits, (const int8_t *)f->d_tmpl, f->sa, 1,
                           L, mh, d_counts, d_idx, d_sc);
    } else {
        const size_t need = (size_t)2 * nseg * sizeof(int);
        if (f->cap_seg < need) {
            HIPCHK(hipStreamSynchronize(f->stream));
            HIPCHK(reserve(f->d_seg, f->cap_seg, need, need, hip_malloc));
        }
        int *segcnt = f->d_seg, *segoff = f->d_seg + nseg;
        for (int t = 0; t < K; ++t) {
            const int Tt = f->T[t];
            const int ns = (L + Tt - 1 + SYNC_SEG - 1) / SYNC_SEG;
            const size_t lds = (size_t)Tt + SYNC_SEG + Tt - 1;
            const int8_t *tp = f->d_tmpl + f->sa.toff[t];
            hipLaunchKernelGGL((k_sync_find<false>), dim3(ns, 1), dim3(256), lds, f->stream, (const uint8_t *)f->d_bits, tp, L, Tt, f->thr[t], ns,
                               segcnt, (const int *)nullptr, mh, (int32_t *)nullptr, (int32_t *)nullptr);
            hipLaunchKernelGGL(k_sync_scan, dim3(1), dim3(64), 0, f->stream, (const int *)segcnt, segoff, d_counts + t, 1, ns);
            hipLaunchKernelGGL((k_sync_find<true>), dim3(ns, 1), dim3(256), lds, f->stream, (const uint8_t *)f->d_bits, tp, L, Tt, f->thr[t], ns,
                               segcnt, (const int *)segoff, mh, d_idx + (size_t)t * mh, d_sc + (size_t)t * mh);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(f->h_res, f->d_res, (size_t)K * (1 + 2 * (size_t)mh) * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipEventRecord(f->done, f->stream));
    f->busy = true;
    return MFB_OK;
}

extern "C" int mfb_syncfinder_end(mfb_syncfinder *f, int32_t *counts, int32_t *hit_idx, int32_t *hit_score) {
    if (!f || !counts || !hit_idx || !hit_score) return MFB_ERR_ARG;
    if (!f->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(f->device));
    const int rc = f->finish();        // (begin has put the copy to h_res on the stream)
    if (rc) return rc;
    const int K = f->K, mh = f->max_hits;
    const int32_t *r = f->h_res;
    memcpy(counts, r, (size_t)K * sizeof(int32_t));
    for (int t = 0; t < K; ++t) {
        const int n = r[t] < mh ? r[t] : mh;
        memcpy(hit_idx + (size_t)t * mh, r + K + (size_t)t * mh, (size_t)n * sizeof(int32_t));
        memcpy(hit_score + (size_t)t * mh, r + K + (size_t)K * mh + (size_t)t * mh, (size_t)n * sizeof(int32_t));
    }
    return MFB_OK;
}

// ---- packed sync correlation (sync_kernels.hpp, second half)-------------------------------------------------------------
// One page-locked buffer per device, grown on demand: callers that produce their packed bit streams straight into it
// (mfb_sync_pinned_buffer) get a true asynchronous host-to-device copy; any other host pointer works too (the runtime stages it).
static std::mutex g_pin_mu;
static HostBuf<uint8_t> *const g_pin = new HostBuf<uint8_t>[SYNC_MAX_DEVICES];     // never deleted: they live until the process exits, as before
static size_t g_pin_cap[SYNC_MAX_DEVICES];

extern "C" int mfb_sync_pinned_buffer(int device, size_t bytes, void **host) {
    if (!host || bytes < 1) return MFB_ERR_ARG;
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    HIPCHK(reserve(g_pin[device], g_pin_cap[device], bytes, bytes, hip_host_malloc));
    *host = g_pin[device];
    return MFB_OK;
}

extern "C" int mfb_sync_find_packed(int device, const uint8_t *packed, int B, int L, int row_bytes, const int8_t *tmpl, int T,
                                    int threshold, int max_total, int32_t *hit_idx, int32_t *hit_score, int32_t *counts,
                                    int32_t *total_hits, float *device_ms) {
    if (!packed || !tmpl || !hit_idx || !hit_score || !counts || !total_hits || B < 1 || L < 1 || T < 1 || T > 64 * SYNCP_MAXK ||
        max_total < 1 || row_bytes < (L + 7) / 8)
        return MFB_ERR_ARG;
    const int K = (T + 63) / 64;
    std::vector<unsigned long long> masks(2 * (size_t)K, 0ull);
    for (int t = 0; t < T; ++t) {
        if (tmpl[t] == 1) masks[t / 64] |= 1ull << (t % 64);
        else if (tmpl[t] == -1) masks[K + t / 64] |= 1ull << (t % 64);
        else if (tmpl[t] != 0) return MFB_ERR_UNSUPPORTED;       // the packed form takes taps in {-1, 0, +1} only
    }
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    WsLease lease{device, ws_acquire(device)};
    if (!lease.w) return MFB_ERR_HIP;
    SyncWs &w = *lease.w;
    const int nseg = (L + T - 1 + SYNCP_SEG - 1) / SYNCP_SEG;
    const size_t nbytes = (size_t)B * row_bytes;
    if ((rc = ws_reserve(&w.bits, &w.cap_bits, nbytes))) return rc;
    if ((rc = ws_reserve(&w.tmpl, &w.cap_tmpl, masks.size() * sizeof(unsigned long long)))) return rc;
    if ((rc = ws_reserve(&w.seg, &w.cap_seg, ((size_t)2 * B * nseg + 2 * (size_t)B + 1) * sizeof(int)))) return rc;
    if ((rc = ws_reserve(&w.hits, &w.cap_hits, (size_t)2 * max_total * sizeof(int32_t)))) return rc;
    if ((rc = ws_reserve(&w.d_stage, &w.cap_dstage, (size_t)B * nseg * SYNCP_THREADS))) return rc;       // hits per thread, one byte
    int *segcnt = w.seg, *segoff = segcnt + (size_t)B * nseg, *d_counts = segoff + (size_t)B * nseg, *d_streamoff = d_counts + B;
    int32_t *d_idx = w.hits, *d_sc = w.hits + max_total;
    uint8_t *d_tcnt = w.d_stage;
    Event e0, e1;
    if (device_ms) {
        HIPCHK(hipEventCreate(out(e0)));
        HIPCHK(hipEventCreate(out(e1)));
    }
    HIPCHK(hipMemcpyAsync(w.bits, packed, nbytes, hipMemcpyHostToDevice, w.stream));
    HIPCHK(hipMemcpyAsync(w.tmpl, masks.data(), masks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, w.stream));
    if (e0) HIPCHK(hipEventRecord(e0, w.stream));
    const unsigned long long *d_masks = (const unsigned long long *)w.tmpl.get();
#define SYNCP_LAUNCH(WRITE_, KT_)                                                                                                        \
    hipLaunchKernelGGL((k_sync_packed<WRITE_, KT_>), dim3(nseg, B), dim3(SYNCP_THREADS), 0, w.stream, (const uint8_t *)w.bits, row_bytes, L, T, \
                       K, d_masks, threshold, nseg, segcnt, d_tcnt, (const int *)segoff, (const int *)d_streamoff, max_total, d_idx, d_sc)
    if (K == 1) SYNCP_LAUNCH(false, 1);
    else if (K == 2) SYNCP_LAUNCH(false, 2);
    else SYNCP_LAUNCH(false, 0);
    hipLaunchKernelGGL(k_sync_scan, dim3((B + 63) / 64), dim3(64), 0, w.stream, (const int *)segcnt, segoff, d_counts, B, nseg);
    hipLaunchKernelGGL(k_sync_stream_scan, dim3(1), dim3(256), 0, w.stream, (const int *)d_counts, d_streamoff, B);
    if (K == 1) SYNCP_LAUNCH(true, 1);
    else if (K == 2) SYNCP_LAUNCH(true, 2);
    else SYNCP_LAUNCH(true, 0);
#undef SYNCP_LAUNCH
    HIPCHK(hipGetLastError());
    if (e1) HIPCHK(hipEventRecord(e1, w.stream));
    // counts and the grand total first, then exactly the hits
    std::vector<int> hc((size_t)2 * B + 1);
    HIPCHK(hipMemcpyAsync(hc.data(), d_counts, hc.size() * sizeof(int), hipMemcpyDeviceToHost, w.stream));
    HIPCHK(hipStreamSynchronize(w.stream));
    memcpy(counts, hc.data(), (size_t)B * sizeof(int));
    const int total = hc[(size_t)2 * B];
    *total_hits = total;
    const int n = total < max_total ? total : max_total;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(hit_idx, d_idx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipMemcpyAsync(hit_score, d_sc, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, w.stream));
        HIPCHK(hipStreamSynchronize(w.stream));
    }
    if (device_ms) HIPCHK(hipEventElapsedTime(device_ms, e0, e1));
    return MFB_OK;
}
