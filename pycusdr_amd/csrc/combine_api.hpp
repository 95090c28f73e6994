// combine_api.hpp -- the host side of the soft combiner (mfb_combiner_*) and its test seams.
// A part of mfbank.hip's one translation unit: included there once, behind combine_kernels.hpp and stage_handle.hpp.  Host code only.
#pragma once

// ---- the soft combiner (combine_kernels.hpp) --------------------------------------------------------------------------------
// A combiner keeps a stream, page-locked staging and device buffers of its own, like the sync finder above.  Staging layout, host
// and device alike: master bits | master trust | slave 0 bits | slave 0 trust | ...; results: mfb_combine_result | bits | trust.
#define CMB_MAX_BITS (1 << 20)
struct mfb_combiner : StageHandle {
    int max_bits = 0, max_slaves = 0;
    HostBuf<uint8_t> h_in, h_out;
    DevBuf<uint8_t> d_in, d_out;
    DevBuf<uint32_t> d_mw, d_sw;
    DevBuf<int32_t> d_x;
    DevBuf<cmb_key> d_cand;
    DevBuf<uint8_t> d_lut;
    int lut_set = 0;           // bit v: the table for v voters is set
    int Lm = 0;
};

static int cmb_pow2ceil(int n) {
    int N = 1;
    while (N < n) N <<= 1;
    return N;
}

// pack -> zero x -> correlate -> per-workgroup candidates, all on `s`; returns the number of candidates through *ncand
static int cmb_enqueue_xcorr(hipStream_t s, const uint8_t *d_slave, int n, int Lmax, const uint32_t *d_mw, uint32_t *d_sw, int32_t *d_x,
                             cmb_key *d_cand, const mfb_combine_result *d_res, int Lfix, int *ncand) {
    const int N = cmb_pow2ceil(n);
    const int NW = N >= 32 ? N / 32 : 1;
    hipLaunchKernelGGL(k_cmb_pack, dim3((NW * 32 + 255) / 256), dim3(256), 0, s, d_slave, n, (uint32_t)(N - 1), d_sw, NW);
    HIPCHK(hipMemsetAsync(d_x, 0, (size_t)N * sizeof(int32_t), s));
    const int L = Lmax < n ? Lmax : n;
    const int tiles = ((L + 31) / 32 + CMB_TILE - 1) / CMB_TILE;
    const int gx = (NW + CMB_QB - 1) / CMB_QB;
    int gy = 1024 / gx;
    gy = gy < 1 ? 1 : gy > tiles ? tiles : gy;
    hipLaunchKernelGGL(k_cmb_xcorr, dim3(gx, gy), dim3(256), 0, s, d_mw, (const uint32_t *)d_sw, (uint32_t)(NW - 1), n, N, d_res, Lfix, d_x);
    if (d_cand) {
        const int g = (N + CMB_SEG - 1) / CMB_SEG;
        hipLaunchKernelGGL(k_cmb_top_seg, dim3(g), dim3(256), 0, s, (const int32_t *)d_x, N, d_res, d_cand);
        *ncand = g * CMB_TOPK;
    }
    HIPCHK(hipGetLastError());
    return MFB_OK;
}

extern "C" int mfb_combiner_destroy(mfb_combiner *c) { return stage_destroy(c); }

static int cmb_create_impl(mfb_combiner *c) {
    const size_t in_bytes = (size_t)2 * c->max_bits * (1 + c->max_slaves);
    const size_t out_bytes = sizeof(mfb_combine_result) + (size_t)2 * c->max_bits;
    const int N = cmb_pow2ceil(c->max_bits);
    HIPCHK(c->d_in.alloc(in_bytes, dev_alloc));
    HIPCHK(c->h_in.alloc(in_bytes, hip_host_malloc));
    HIPCHK(c->d_out.alloc(out_bytes, dev_alloc));
    HIPCHK(c->h_out.alloc(out_bytes, hip_host_malloc));
    HIPCHK(c->d_mw.alloc(((size_t)c->max_bits / 32 + 2) * sizeof(uint32_t), dev_alloc));
    HIPCHK(c->d_sw.alloc(((size_t)N / 32 + 2) * sizeof(uint32_t), dev_alloc));
    HIPCHK(c->d_x.alloc((size_t)N * sizeof(int32_t), dev_alloc));
    HIPCHK(c->d_cand.alloc((size_t)(CMB_MAX_BITS / CMB_SEG) * CMB_TOPK * sizeof(cmb_key), dev_alloc));
    HIPCHK(c->d_lut.alloc((size_t)3 * CMB_LUT_STRIDE, dev_alloc));
    HIPCHK(hipMemset(c->d_lut, 0, (size_t)3 * CMB_LUT_STRIDE));
    return MFB_OK;
}

extern "C" int mfb_combiner_create(mfb_combiner **out, int device, int max_bits, int max_slaves) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (max_bits < 1 || max_slaves < 0) return MFB_ERR_ARG;
    if (max_bits > CMB_MAX_BITS || max_slaves > MFB_COMBINE_MAX_SLAVES) return MFB_ERR_UNSUPPORTED;
    return stage_create(out, device, [&](mfb_combiner *c) {
        c->max_bits = max_bits;
        c->max_slaves = max_slaves;
        return cmb_create_impl(c);
    });
}

extern "C" int mfb_combiner_set_vote(mfb_combiner *c, int voters, const uint8_t *lut_bits, const int8_t *lut_trust, int entries) {
    if (!c || !lut_bits || !lut_trust || voters < 2 || voters > MFB_COMBINE_MAX_SLAVES + 1 || entries != 1 << (3 * voters)) return MFB_ERR_ARG;
    if (c->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    uint8_t *t = c->d_lut + (size_t)(voters - 2) * CMB_LUT_STRIDE;
    HIPCHK(hipMemcpy(t, lut_bits, (size_t)entries, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t + 4096, lut_trust, (size_t)entries, hipMemcpyHostToDevice));
    c->lut_set |= 1 << voters;
    return MFB_OK;
}

extern "C" int mfb_combiner_begin(mfb_combiner *c, const mfb_combine_params *p, const uint8_t *master_bits, const int8_t *master_trust,
                                  const uint8_t *const *slave_bits, const int8_t *const *slave_trust) {
    if (!c || !p || !master_bits || !master_trust) return MFB_ERR_ARG;
    const int ns = p->num_slaves, Lm = p->master_len;
    if (ns < 0 || Lm < 1 || Lm > c->max_bits) return MFB_ERR_ARG;
    if (ns > MFB_COMBINE_MAX_SLAVES) return MFB_ERR_UNSUPPORTED;
    if (ns > c->max_slaves || (ns > 0 && (!slave_bits || !slave_trust))) return MFB_ERR_ARG;
    for (int i = 0; i < ns; ++i)
        if (p->slave_len[i] < 1 || p->slave_len[i] > c->max_bits || !slave_bits[i] || !slave_trust[i]) return MFB_ERR_ARG;
    if (c->busy) return MFB_ERR_STATE;
    for (int v = 2; v <= ns + 1; ++v)
        if (!(c->lut_set & (1 << v))) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    // one packed copy in
    size_t off = 0, soff[MFB_COMBINE_MAX_SLAVES] = {};
    memcpy(c->h_in, master_bits, (size_t)Lm);
    memcpy(c->h_in + Lm, master_trust, (size_t)Lm);
    off = (size_t)2 * Lm;
    for (int i = 0; i < ns; ++i) {
        const size_t n = (size_t)p->slave_len[i];
        soff[i] = off;
        memcpy(c->h_in + off, slave_bits[i], n);
        memcpy(c->h_in + off + n, slave_trust[i], n);
        off += 2 * n;
    }
    HIPCHK(hipMemcpyAsync(c->d_in, c->h_in, off, hipMemcpyHostToDevice, c->stream));
    mfb_combine_result *d_res = (mfb_combine_result *)c->d_out.get();
    hipLaunchKernelGGL(k_cmb_init, dim3(1), dim3(64), 0, c->stream, d_res, Lm, ns);
    const int MW = (Lm + 31) / 32;
    hipLaunchKernelGGL(k_cmb_pack, dim3((MW * 32 + 255) / 256), dim3(256), 0, c->stream, (const uint8_t *)c->d_in, Lm, 0xFFFFFFFFu, c->d_mw, MW);
    CmbVoteArgs va = {};
    for (int i = 0; i < ns; ++i) {
        const int n = p->slave_len[i];
        va.bits[i] = c->d_in + soff[i];
        va.trust[i] = (const int8_t *)(c->d_in + soff[i] + n);
        va.n[i] = n;
        if (n < 16) continue;          // not evaluated, not matched (mfbank.h)
        int ncand = 0;
        const int rc = cmb_enqueue_xcorr(c->stream, va.bits[i], n, Lm, c->d_mw, c->d_sw, c->d_x, c->d_cand, d_res, 0, &ncand);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cmb_decide, dim3(1), dim3(256), 0, c->stream, (const cmb_key *)c->d_cand, ncand, d_res, i, n, p->variance_multiplier,
                           p->min_length);
    }
    uint8_t *d_ob = c->d_out + sizeof(mfb_combine_result);
    hipLaunchKernelGGL(k_cmb_vote, dim3((Lm + 255) / 256), dim3(256), 0, c->stream, (const mfb_combine_result *)d_res, (const uint8_t *)c->d_in,
                       (const int8_t *)(c->d_in + Lm), va, (const uint8_t *)c->d_lut, d_ob, (int8_t *)(d_ob + Lm));
    hipLaunchKernelGGL(k_cmb_finish, dim3(1), dim3(1), 0, c->stream, d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, sizeof(mfb_combine_result) + (size_t)2 * Lm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->done, c->stream));
    c->Lm = Lm;
    c->busy = true;
    return MFB_OK;
}

extern "C" int mfb_combiner_end(mfb_combiner *c, mfb_combine_result *result, uint8_t *bits, int8_t *trust) {
    if (!c || !result || !bits || !trust) return MFB_ERR_ARG;
    if (!c->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const int rc = c->finish();        // (begin has put the copy to h_out on the stream)
    if (rc) return rc;
    memcpy(result, c->h_out, sizeof(mfb_combine_result));
    const int L = result->out_len;
    if (L < 0 || L > c->Lm) return MFB_ERR_HIP;
    memcpy(bits, c->h_out + sizeof(mfb_combine_result), (size_t)L);
    memcpy(trust, c->h_out + sizeof(mfb_combine_result) + c->Lm, (size_t)L);
    return MFB_OK;
}

extern "C" int mfb_debug_bit_xcorr(int device, const uint8_t *a_bits, int n, const uint8_t *b_bits, int m, int32_t *out) {
    if (!a_bits || !b_bits || !out || n < 1 || m < 1) return MFB_ERR_ARG;
    if (n > CMB_MAX_BITS || m > CMB_MAX_BITS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    const int N = cmb_pow2ceil(n), MW = (m + 31) / 32;
    DevBuf<uint8_t> d_a, d_b;
    DevBuf<uint32_t> d_mw, d_sw;
    DevBuf<int32_t> d_x;
    HIPCHK(d_a.alloc((size_t)n, hip_malloc));
    HIPCHK(d_b.alloc((size_t)m, hip_malloc));
    HIPCHK(d_mw.alloc(((size_t)MW + 2) * sizeof(uint32_t), hip_malloc));
    HIPCHK(d_sw.alloc(((size_t)N / 32 + 2) * sizeof(uint32_t), hip_malloc));
    HIPCHK(d_x.alloc((size_t)N * sizeof(int32_t), hip_malloc));
    HIPCHK(hipMemcpy(d_a, a_bits, (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_b, b_bits, (size_t)m, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cmb_pack, dim3((MW * 32 + 255) / 256), dim3(256), 0, nullptr, (const uint8_t *)d_b, m, 0xFFFFFFFFu, d_mw, MW);
    int ncand = 0;
    const int rc2 = cmb_enqueue_xcorr(nullptr, d_a, n, m, d_mw, d_sw, d_x, nullptr, nullptr, m, &ncand);
    if (rc2) return rc2;
    HIPCHK(hipMemcpy(out, d_x, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MFB_OK;
}

// Test seam of the peak stages: what a call runs for slave 0 after its correlation -- init, top-15 per segment, merge and decision,
// finish: the same kernels, the same grids -- on a correlation x[nlags] of the caller's choice.  No streams, so no vote.
extern "C" int mfb_debug_combine_peaks(int device, const int32_t *x, int nlags, int n, int master_len, double variance_multiplier,
                                       int min_length, mfb_combine_result *out) {
    if (!x || !out || nlags < 1 || n < 1 || master_len < 1) return MFB_ERR_ARG;
    if (nlags > CMB_MAX_BITS || n > CMB_MAX_BITS || master_len > CMB_MAX_BITS) return MFB_ERR_UNSUPPORTED;
    for (int i = 0; i < nlags; ++i)
        if (x[i] < 0) return MFB_ERR_ARG;
    int rc = device_ok(device, SYNC_MAX_DEVICES);
    if (rc) return rc;
    const int g = (nlags + CMB_SEG - 1) / CMB_SEG;
    DevBuf<int32_t> d_x;
    DevBuf<cmb_key> d_cand;
    DevBuf<mfb_combine_result> d_res;
    HIPCHK(d_x.alloc((size_t)nlags * sizeof(int32_t), hip_malloc));
    HIPCHK(d_cand.alloc((size_t)g * CMB_TOPK * sizeof(cmb_key), hip_malloc));
    HIPCHK(d_res.alloc(sizeof(mfb_combine_result), hip_malloc));
    HIPCHK(hipMemcpy(d_x, x, (size_t)nlags * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cmb_init, dim3(1), dim3(64), 0, nullptr, d_res, master_len, 1);
    hipLaunchKernelGGL(k_cmb_top_seg, dim3(g), dim3(256), 0, nullptr, (const int32_t *)d_x, nlags, (const mfb_combine_result *)d_res, d_cand);
    hipLaunchKernelGGL(k_cmb_decide, dim3(1), dim3(256), 0, nullptr, (const cmb_key *)d_cand, g * CMB_TOPK, d_res, 0, n, variance_multiplier,
                       min_length);
    hipLaunchKernelGGL(k_cmb_finish, dim3(1), dim3(1), 0, nullptr, d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_res, sizeof(mfb_combine_result), hipMemcpyDeviceToHost));
    return MFB_OK;
}
