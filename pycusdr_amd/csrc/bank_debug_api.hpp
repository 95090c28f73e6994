// bank_debug_api.hpp -- the bank's test seams (mfb_debug_*): product launches on injected data, and the planner's answer for a handle.
// A part of mfbank.hip's one translation unit: included there once, last of the bank's parts.  Host code only.
#pragma once

extern "C" int mfb_debug_search_plan(mfb_ctx *c, mfb_plan_inputs *inputs, int nblocks, mfb_search_plan *out) {
    if (!inputs || !out || nblocks < 1) return MFB_ERR_ARG;
    if (c && !c->have_filters) return MFB_ERR_STATE;
    if (c) *inputs = search_inputs(c);
    const Segments sg = c ? segments(c) : resolve_segments(*inputs);
    if (!sg.ok) return MFB_ERR_UNSUPPORTED;
    *out = plan_search(*inputs, sg, nblocks);
    if (sg.path == MFB_PATH_SEGMENT) out->store = plan_store(*inputs, sg, nblocks);     // ... and the matched-filter pass of the same blocks
    return MFB_OK;
}

// Test seam of the stream stages (include/mfbank.h): k_stream_align / _sync / _ring / _edges on INJECTED symbol decisions.
extern "C" int mfb_debug_stream_stages(mfb_ctx *c, int nb, int symbols, const int32_t *counts, const int32_t *sym, const int32_t *cen,
                                       const float *mag, void *dst, size_t capacity, mfb_record_layout *lay) {
    if (!c || nb < 1 || nb > 64 || symbols < 1 || !counts || !sym || !cen || !mag || !dst || !lay) return MFB_ERR_ARG;
    if (!c->st_on) return MFB_ERR_STATE;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const RecordLayout l = rec_layout(0, symbols, true);
    const size_t rec = l.bytes;
    if (capacity < rec * (size_t)nb) return MFB_ERR_ARG;
    int rc = batch_reserve(c, nb > c->bat_cap ? nb : (c->bat_cap > 0 ? c->bat_cap : nb), rec);
    if (rc) return rc;
    if (rec * nb > c->batout_cap) return MFB_ERR_ALLOC;
    std::vector<uint8_t> h(rec * (size_t)nb, 0);
    for (int b = 0; b < nb; ++b) {
        if (counts[b] < 0 || counts[b] > symbols) return MFB_ERR_ARG;
        uint8_t *r = h.data() + (size_t)b * rec;
        BlockScalars sc;
        memset(&sc, 0, sizeof(sc));
        sc.count = counts[b];
        memcpy(r + l.scalars, &sc, sizeof(sc));
        memcpy(r + l.sym, sym + (size_t)b * symbols, (size_t)symbols * sizeof(int));
        memcpy(r + l.cen, cen + (size_t)b * symbols, (size_t)symbols * sizeof(int));
        memcpy(r + l.mag, mag + (size_t)b * symbols, (size_t)symbols * sizeof(float));
    }
    HIPCHK(hipMemcpyAsync(c->d_batout, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = stream_stages_enqueue(c, c->d_batout, l, nb, symbols, c->carry_cur, nullptr))) return rc;
    c->carry_cur = 1 - c->carry_cur;
    HIPCHK(hipMemcpyAsync(dst, c->d_batout, rec * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    fill_layout(lay, c, l, nb, symbols, 0, MFB_BLOCK_SEARCH, 0);
    return MFB_OK;
}

// Test seam of the one-call path (include/mfbank.h): block_pick_body / block_rate_body on injected device results.
extern "C" int mfb_debug_block_scalars(mfb_ctx *c, int n, const float *picks, const float *triples, int spsym_min, int snr_window,
                                       int max_symbols, mfb_block_result *results, float *launch_args, int32_t *band_pieces) {
    if (!c || n < 1 || !picks || !triples || !results || spsym_min < 2 || snr_window < 0 || max_symbols < 1) return MFB_ERR_ARG;
    if (!c->have_shifts) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    DevBuf<float> d_in;
    DevBuf<BlockScalars> d_out;
    std::vector<BlockScalars> h((size_t)n);
    const size_t in_bytes = (size_t)n * 5 * sizeof(float);
    if (d_in.alloc(in_bytes, hip_malloc) != hipSuccess || d_out.alloc((size_t)n * sizeof(BlockScalars), hip_malloc) != hipSuccess) return MFB_ERR_ALLOC;
    if (hipMemcpy(d_in, picks, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in + 2 * (size_t)n, triples, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return MFB_ERR_HIP;
    const int capacity = max_symbols < c->cap ? max_symbols : c->cap;
    hipLaunchKernelGGL(k_block_scalars_debug, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, (const float *)d_in,
                       (const float *)(d_in + 2 * (size_t)n), (const int *)c->d_shifts, c->Dtot, c->N, snr_window, spsym_min, capacity,
                       d_out);
    if (hipGetLastError() != hipSuccess || sync_streams(c) != hipSuccess ||
        hipMemcpy(h.data(), d_out, (size_t)n * sizeof(BlockScalars), hipMemcpyDeviceToHost) != hipSuccess)
        return MFB_ERR_HIP;
    for (int i = 0; i < n; ++i) {
        const BlockScalars &hs = h[(size_t)i];
        fill_result(&results[i], hs, MFB_BLOCK_SEARCH, 0);
        if (launch_args) {
            launch_args[2 * i] = hs.spSymF;
            launch_args[2 * i + 1] = hs.offsetF;
        }
        if (band_pieces) memcpy(band_pieces + 8 * (size_t)i, &hs.band[0][0][0], 8 * sizeof(int32_t));
    }
    return MFB_OK;
}

// Test seam: k_unpack on nsamples host samples, the complex64 result back to the host.  The product paths do not come here.
extern "C" int mfb_debug_unpack(int device, int format, float scale, const void *raw, size_t nsamples, float *out_c64) {
    if (!raw || !out_c64 || nsamples < 1 || nsamples > ((size_t)1 << 28) || (format != MFB_SAMPLES_SC16 && format != MFB_SAMPLES_SC8))
        return MFB_ERR_ARG;
    const float sc = fmt_scale_checked(format, scale);
    if (sc == 0.f) return MFB_ERR_ARG;
    const int rc = device_ok(device);
    if (rc) return rc;
    const size_t bytes = nsamples * (size_t)sample_bytes(format);
    DevBuf<void> d_in;
    DevBuf<cf> d_out;
    HIPCHK(d_in.alloc((bytes + 15) & ~(size_t)15, hip_malloc));
    HIPCHK(d_out.alloc(nsamples * sizeof(cf), hip_malloc));
    HIPCHK(hipMemcpy(d_in, raw, bytes, hipMemcpyHostToDevice));
    const int r = launch_unpack(format, d_in, d_out, nsamples, sc, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(out_c64, d_out, nsamples * sizeof(cf), hipMemcpyDeviceToHost));
    return MFB_OK;
}

// Test seams of the demodulation tail: k_envelope, k_code_rate / k_code_rate_block and k_centres, launched as the product launches
// them, on INJECTED inputs.  Handle-less: buffers of their own on the null stream, a synchronous copy back.
#define DBG_TAIL_MAX_ELEMS ((size_t)1 << 26)      // complex64 elements a seam takes (512 MiB)
extern "C" int mfb_debug_envelope(int device, const float *xc_c64, int nb, int M, int N, int off, float *env) {
    if (!xc_c64 || !env || nb < 1 || M < 1 || N < 1 || off < 0 || 2 * off >= M) return MFB_ERR_ARG;
    if (nb > 65535 || (size_t)nb * (size_t)M * (size_t)N > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const size_t nin = (size_t)nb * M * N, nout = (size_t)nb * N;
    DevBuf<cf> d_xc;
    DevBuf<float> d_env;
    HIPCHK(d_xc.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_env.alloc(nout * sizeof(float), hip_malloc));
    HIPCHK(hipMemcpy(d_xc, xc_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_env, 0x5a, nout * sizeof(float)));
    hipLaunchKernelGGL(k_envelope, dim3(1024, nb), dim3(256), 0, nullptr, (const cf *)d_xc, d_env, N, M, off);     // as demod_enqueue
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(env, d_env, nout * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

// k_band_means on an injected spectrum X[N] and n injected windows, one launch
extern "C" int mfb_debug_band_means(int device, const float *X_c64, int N, int n, const int32_t *pieces, float *means) {
    if (!X_c64 || !pieces || !means || N < 1 || n < 1) return MFB_ERR_ARG;
    if (n > 65535 || N > SNR_MAX_CHUNKS * SNR_CHUNK) return MFB_ERR_UNSUPPORTED;      // (the largest block: 2^22)
    for (int i = 0; i < n; ++i) {
        const int32_t *q = pieces + 4 * (size_t)i;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || (long long)q[0] + q[1] > N || (long long)q[2] + q[3] > N ||
            (long long)q[1] + q[3] > N)
            return MFB_ERR_ARG;
    }
    int rc = device_ok(device);
    if (rc) return rc;
    DevBuf<cf> d_X;
    DevBuf<int> d_p;
    DevBuf<float> d_m;
    HIPCHK(d_X.alloc((size_t)N * sizeof(cf), hip_malloc));
    HIPCHK(d_p.alloc((size_t)n * 4 * sizeof(int), hip_malloc));
    HIPCHK(d_m.alloc((size_t)n * sizeof(float), hip_malloc));
    HIPCHK(hipMemcpy(d_X, X_c64, (size_t)N * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_p, pieces, (size_t)n * 4 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_m, 0x5a, (size_t)n * sizeof(float)));
    hipLaunchKernelGGL(k_band_means, dim3(1, n), dim3(SNR_THREADS), 0, nullptr, (const float2 *)d_X.get(), (size_t)0, N, (const int *)d_p,
                       4 * sizeof(int), d_m, sizeof(float));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(means, d_m, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

#define DBG_REC_STRIDE 256       // bytes from one window's BlockScalars to the next (static_assert: sizeof(BlockScalars) <= 256)
extern "C" int mfb_debug_code_rate(int device, const float *P_c64, int nb, int n, int offset, int len, int spsym_min, int capacity,
                                   float *triples, float *block_triples, double *rate, float *launch_args, int32_t *counts) {
    if (!P_c64 || !triples || !block_triples || !rate || !launch_args || !counts || nb < 1 || n < 1) return MFB_ERR_ARG;
    if (offset < 0 || len < 0 || (long long)offset + len > n) return MFB_ERR_ARG;          // as mfb_demodulate
    if (nb > 65535 || (size_t)nb * (size_t)n > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const size_t nin = (size_t)nb * n;
    DevBuf<cf> d_P;
    DevBuf<float> d_cr;              // [2][nb][3]: k_code_rate's triples, then k_code_rate_block's
    DevBuf<uint8_t> d_sc;
    std::vector<uint8_t> recs((size_t)nb * DBG_REC_STRIDE);
    HIPCHK(d_P.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_cr.alloc((size_t)6 * nb * sizeof(float), hip_malloc));
    HIPCHK(d_sc.alloc(recs.size(), hip_malloc));
    HIPCHK(hipMemcpy(d_P, P_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_cr, 0x5a, (size_t)6 * nb * sizeof(float)));
    HIPCHK(hipMemset(d_sc, 0, recs.size()));
    for (int b = 0; b < nb; ++b)
        hipLaunchKernelGGL(k_code_rate, dim3(1), dim3(1024), 0, nullptr, (const cf *)(d_P + (size_t)b * n), d_cr + 3 * (size_t)b, offset,
                           len);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_code_rate_block, dim3(nb), dim3(1024), 0, nullptr, (const cf *)d_P, d_cr + 3 * (size_t)nb, offset, len, n,
                       spsym_min, capacity, reinterpret_cast<BlockScalars *>(d_sc.get()), (size_t)DBG_REC_STRIDE);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(triples, d_cr, (size_t)3 * nb * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(block_triples, d_cr + 3 * (size_t)nb, (size_t)3 * nb * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(recs.data(), d_sc, recs.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) {
        BlockScalars sc;
        memcpy(&sc, recs.data() + (size_t)b * DBG_REC_STRIDE, sizeof(sc));
        rate[2 * b] = sc.spSym;
        rate[2 * b + 1] = sc.codeOffset;
        launch_args[2 * b] = sc.spSymF;
        launch_args[2 * b + 1] = sc.offsetF;
        counts[2 * b] = sc.count;
        counts[2 * b + 1] = sc.rate_fallback;
    }
    return MFB_OK;
}

extern "C" int mfb_debug_centres(int device, const float *sig_c64, int M, int lenSig, int W, int op, float spSym, float offset,
                                 int capacity, int nthreads, int32_t *sym, int32_t *cen, float *mag) {
    if (!sig_c64 || !sym || !cen || !mag || M < 1 || lenSig < 1 || W < 1 || op < 0 || op > 2 || capacity < 0 || nthreads < 1)
        return MFB_ERR_ARG;
    if (!(spSym >= 2.0f) || !(offset >= 0.f) || !(offset < 2147483648.f)) return MFB_ERR_ARG;       // as mfb_find_centres; a code phase is >= 0
    if (nthreads > (1 << 20) || lenSig > (1 << 22) || (size_t)M * (size_t)lenSig > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const int nblk = (nthreads + 255) / 256;
    const size_t nin = (size_t)M * lenSig, nent = (size_t)nblk * 256;
    DevBuf<cf> d_sig;
    DevBuf<int32_t> d_out;           // [3][nent]: sym, cen, mag
    HIPCHK(d_sig.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_out.alloc(3 * nent * sizeof(int32_t), hip_malloc));
    HIPCHK(hipMemcpy(d_sig, sig_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0x5a, 3 * nent * sizeof(int32_t)));        // the canary: what the kernel leaves alone stays 0x5a5a5a5a
    hipLaunchKernelGGL(k_centres, dim3(nblk), dim3(256), 0, nullptr, (int *)d_out, (int *)(d_out + nent),
                       reinterpret_cast<float *>(d_out + 2 * nent), (const cf *)d_sig, spSym, offset, lenSig, M, W, op, capacity);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(sym, d_out, nent * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cen, d_out + nent, nent * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mag, d_out + 2 * nent, nent * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

#ifdef MFB_SEG_TRACE
extern "C" int mfb_debug_read_trace(unsigned long long *out, int nblocks) {
    if (!out || nblocks < 1 || nblocks > 65536) return MFB_ERR_ARG;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seg_trace), (size_t)nblocks * 3 * sizeof(unsigned long long)));
    return MFB_OK;
}
#endif
