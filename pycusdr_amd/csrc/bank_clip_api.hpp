// bank_clip_api.hpp -- interference-peak clipping in front of a bank's forward transform (mfb_set_peak_clip; the kernels: clip_kernels.hpp).
// A part of mfbank.hip's one translation unit: included there once, behind bank_ctx.hpp.  Host code only.
#pragma once

// ---- interference-peak clipping (clip_kernels.hpp; reference __thresholdInput, DB:670-707) -----------------------------------
struct ClipLaunch {
    ClipArgs a;
    int32_t *h_head;     // page-locked copy of the heads, read back with the flight
};
// buffers of the clip: the flight's own (clipped blocks, indices, heads: slot `slot`, up to nb blocks -- the other slot's flight,
// pending or collected, keeps its own), the shared workspace of part 1 and the chain tail (stable addresses: captured graphs
// hold them)
static int clip_reserve(mfb_ctx *c, int slot, int nb) {
    if (nb > c->clip_cap[slot]) {
        HIPCHK(sync_and_invalidate(c));
        const size_t nbN = (size_t)nb * c->N, heads = (size_t)nb * CLIP_HEAD * sizeof(int);
        const int rc = grow_buffers(&c->clip_cap[slot], 0, {{&c->d_clipx[slot], nbN * sizeof(cf)}, {&c->d_clipi[slot], nbN * sizeof(int)}, {&c->d_cliph[slot], heads}});
        if (rc) return rc;
        HIPCHK(c->h_cliph[slot].alloc(heads, hip_host_malloc));
        memset(c->h_cliph[slot], 0, heads);
        c->clip_cap[slot] = nb;        // (device and host side exist)
    }
    if (nb > c->clip_ws_cap) {       // part 1 only, on the handle's stream: nothing in flight reads it after the wait
        HIPCHK(sync_and_invalidate(c));
        const size_t nbN = (size_t)nb * c->N;
        const int rc = grow_buffers(&c->clip_ws_cap, nb, {{&c->d_clips, (2 * nbN / CLIP_LEAF + 2 * (size_t)nb) * sizeof(float)}, {&c->d_clipw, 2 * nbN / CLIP_WAVE * sizeof(int)}});
        if (rc) return rc;
    }
    if (c->clip_ov > c->ctail_cap) {
        HIPCHK(sync_and_invalidate(c));
        const size_t bytes = sizeof(ClipTail) + (size_t)c->clip_ov * sizeof(cf);
        const int rc = grow_buffers(&c->ctail_cap, 0, {{&c->d_ctail, bytes}});
        if (rc) return rc;
        HIPCHK(hipMemset(c->d_ctail, 0, bytes));
        c->ctail_cap = c->clip_ov;     // (and cleared)
    }
    return MFB_OK;
}
// The clip of nb blocks (block b at raw + b * xstride) for flight `slot`: its arguments, and the chain's restart if one is due
static int clip_prepare(mfb_ctx *c, int slot, const cf *raw, long long xstride, int nb, ClipLaunch *L) {
    // (a window's batches: room for the window's blocks at once, as batch_reserve does, so that sizes 1 ... B share the buffers)
    int rc = clip_reserve(c, slot, nb > c->win_blocks ? nb : (c->win_blocks > 0 && xstride != 0 ? c->win_blocks : nb));
    if (rc) return rc;
    ClipArgs &a = L->a;
    const size_t nbN = (size_t)c->clip_ws_cap * c->N;
    a.x = (const float2 *)raw;
    a.xstride = xstride;
    a.y = (float2 *)c->d_clipx[slot].get();
    a.idx = c->d_clipi[slot];
    a.head = c->d_cliph[slot];
    a.s1 = c->d_clips;
    a.s2 = c->d_clips + nbN / CLIP_LEAF;
    a.thr = c->d_clips + 2 * nbN / CLIP_LEAF;
    a.wcnt = c->d_clipw;
    a.wflag = c->d_clipw + nbN / CLIP_WAVE;
    a.tail = c->clip_ov > 0 ? c->d_ctail : nullptr;
    a.N = c->N;
    a.ov = c->clip_ov;
    a.nb = nb;
    a.scale = c->clip_scale;
    L->h_head = c->h_cliph[slot];
    if (c->clip_restart) {       // outside any captured graph: the next block's overlap is taken as it is
        if (c->d_ctail) HIPCHK(hipMemsetAsync(c->d_ctail, 0, sizeof(int32_t), c->stream));
        c->clip_restart = false;
    }
    return MFB_OK;
}
// sum, sum again, clip, compact for every block at once; the chain in order (ov > 0); the heads to the flight's staging
static int clip_enqueue(mfb_ctx *c, const ClipLaunch &L) {
    const ClipArgs &a = L.a;
    const dim3 grid(c->N / (CLIP_WAVE * (CLIP_THREADS / 64)), a.nb);
    hipLaunchKernelGGL(k_clip_sum1, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_sum2, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_apply, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_compact, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    if (a.tail) hipLaunchKernelGGL(k_clip_chain, dim3(1), dim3(CLIP_CHAIN_THREADS), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(L.h_head, a.head, (size_t)a.nb * CLIP_HEAD * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return MFB_OK;
}
extern "C" int mfb_set_peak_clip(mfb_ctx *c, float scale, int overlap) {
    if (!c || !(scale >= 0.f) || isinf(scale) || overlap < 0 || overlap >= c->N) return MFB_ERR_ARG;
    if (scale > 0.f && c->N < CLIP_THREADS / 64 * CLIP_WAVE) return MFB_ERR_UNSUPPORTED;
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_and_invalidate(c));      // the recorded graphs hold the old settings
    c->clip_scale = scale;
    c->clip_ov = scale > 0.f ? overlap : 0;
    c->clip_restart = true;
    return MFB_OK;
}
extern "C" int mfb_get_peak_clip_tail(mfb_ctx *c, float *host_c64, int count, int32_t *valid) {
    if (!c || !valid || count < 0 || (count > 0 && !host_c64)) return MFB_ERR_ARG;
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    if (c->clip_ov <= 0 || !c->d_ctail || c->clip_restart) {
        *valid = 0;
        return MFB_OK;
    }
    if (count != c->clip_ov) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    HIPCHK(hipMemcpy(valid, &c->d_ctail->valid, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*valid) HIPCHK(hipMemcpy(host_c64, c->d_ctail->s, (size_t)count * sizeof(cf), hipMemcpyDeviceToHost));
    return MFB_OK;
}
extern "C" int mfb_restart_peak_clip(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    c->clip_restart = true;
    return MFB_OK;
}
extern "C" int mfb_get_block_clips(mfb_ctx *c, int slot, int block, int32_t *idx, int cap, int32_t *count) {
    if (!c || slot < 0 || slot > 1 || block < 0 || cap < 0 || !count || (cap > 0 && !idx)) return MFB_ERR_ARG;
    const BlockFlight &f = c->flight[slot];
    if (f.active || !f.clip || block >= (f.nb ? f.nb : 1)) return MFB_ERR_STATE;
    const int32_t *h = c->h_cliph[slot] + (size_t)block * CLIP_HEAD;
    const int n = h[0];
    *count = n;
    const int m = n < cap ? n : cap;
    if (m <= CLIP_HEAD - 1) {
        if (m > 0) memcpy(idx, h + 1, (size_t)m * sizeof(int32_t));
    } else {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpy(idx, c->d_clipi[slot] + (size_t)block * c->N, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return MFB_OK;
}
