// mod_api.hpp -- the host side of the modulator (mfb_modulator_*).
// A part of mfbank.hip's one translation unit: included there once, behind mod_kernels.hpp and stage_handle.hpp.  Host code only.
#pragma once

// ---- the modulator (mod_kernels.hpp) -----------------------------------------------------------------------------------------
// A modulator keeps a stream, page-locked staging and device buffers of its own, like the combiner above.  Staging layout, host
// and device alike: sample_off int64 [B+1] | d uint64 [B] | init uint64 [B] | bit_off int32 [B+1] | bits uint8 -- 8-byte fields first.
#define MOD_MAX_FRAME_BITS (1 << 17)
#define MOD_MAX_FRAMES 4096
#define MOD_MAX_BITS (1 << 22)
#define MOD_MAX_SAMPLES (1 << 24)
struct mfb_modulator : StageHandle {
    int max_bits = 0, max_samples = 0;
    HostBuf<uint8_t> h_in;
    HostBuf<float> h_out;      // on demand (mfb_modulator_host_buffer)
    DevBuf<uint8_t> d_in, d_rows;
    DevBuf<mod_u64> d_symbase, d_P, d_T;
    DevBuf<float2> d_noise, d_out;
    int kind = -1, sps = 0;    // kind < 0: no LUT yet
    int noise_len = 0, pad = 0, min_len = 0;
    bool have = false;         // a finished batch stands in d_out
    int B = 0;
    int64_t total = 0;         // samples of the batch in flight / finished last
    std::vector<int64_t> sample_off;
};

// the quantisation rule of mfbank.h, in IEEE double
static mod_u64 mod_quantise(double v_rad) {
    double t = v_rad / 6.283185307179586;
    t -= floor(t);
    return t >= 1.0 ? 0 : (mod_u64)(t * 18446744073709551616.0);
}

static size_t mod_staging_bytes(int B, int nbits) {
    return (size_t)(B + 1) * 8 + (size_t)B * 16 + (size_t)(B + 1) * 4 + (size_t)nbits;
}

extern "C" int mfb_modulator_destroy(mfb_modulator *m) { return stage_destroy(m); }

static int mod_create_impl(mfb_modulator *m) {
    const int maxB = m->max_bits < MOD_MAX_FRAMES ? m->max_bits : MOD_MAX_FRAMES;
    const size_t in_bytes = mod_staging_bytes(maxB, m->max_bits);
    HIPCHK(m->d_in.alloc(in_bytes, dev_alloc));
    HIPCHK(m->h_in.alloc(in_bytes, hip_host_malloc));
    HIPCHK(m->d_rows.alloc((size_t)m->max_bits, dev_alloc));
    HIPCHK(m->d_symbase.alloc((size_t)m->max_bits * sizeof(mod_u64), dev_alloc));
    HIPCHK(m->d_P.alloc((size_t)MOD_MAX_ROWS * MOD_MAX_SPS * sizeof(mod_u64), dev_alloc));
    HIPCHK(m->d_T.alloc((size_t)MOD_MAX_ROWS * sizeof(mod_u64), dev_alloc));
    HIPCHK(m->d_out.alloc((size_t)m->max_samples * sizeof(float2), dev_alloc));
    HIPCHK(hipMemset(m->d_T, 0, (size_t)MOD_MAX_ROWS * sizeof(mod_u64)));
    return MFB_OK;
}

extern "C" int mfb_modulator_create(mfb_modulator **out, int device, int max_bits, int max_samples) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (max_bits < 1 || max_samples < 1) return MFB_ERR_ARG;
    if (max_bits > MOD_MAX_BITS || max_samples > MOD_MAX_SAMPLES) return MFB_ERR_UNSUPPORTED;
    return stage_create(out, device, [&](mfb_modulator *m) {
        m->max_bits = max_bits;
        m->max_samples = max_samples;
        return mod_create_impl(m);
    });
}

static int mod_set_lut_body(mfb_modulator *m, int kind, const double *lut_rad, int rows, int sps) {
    std::vector<mod_u64> P((size_t)rows * sps), T(MOD_MAX_ROWS, 0);
    for (int r = 0; r < rows; ++r) {
        mod_u64 acc = 0;
        for (int j = 0; j < sps; ++j) {
            const double v = lut_rad[(size_t)r * sps + j];
            if (!std::isfinite(v)) return MFB_ERR_ARG;
            acc += mod_quantise(v);
            P[(size_t)r * sps + j] = acc;
        }
        T[r] = acc;
    }
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));      // nothing in flight, but mfb_debug_mod_phase may have read the old table last
    m->kind = -1;
    m->have = false;                              // the finished batch's rows and scan belong to the old table
    HIPCHK(hipMemcpy(m->d_P, P.data(), P.size() * sizeof(mod_u64), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m->d_T, T.data(), T.size() * sizeof(mod_u64), hipMemcpyHostToDevice));
    m->kind = kind;
    m->sps = sps;
    return MFB_OK;
}

extern "C" int mfb_modulator_set_lut(mfb_modulator *m, int kind, const double *lut_rad, int rows, int sps) {
    if (!m || !lut_rad || (kind != MFB_MOD_FSK && kind != MFB_MOD_GMSK3) || rows != (kind == MFB_MOD_FSK ? 2 : 8) || sps < 1) return MFB_ERR_ARG;
    if (sps < 2 || sps > MOD_MAX_SPS) return MFB_ERR_UNSUPPORTED;
    if (m->busy) return MFB_ERR_STATE;
    return guarded([&] { return mod_set_lut_body(m, kind, lut_rad, rows, sps); });
}

extern "C" int mfb_modulator_set_pad(mfb_modulator *m, const float *noise_iq, int noise_len, int pad_len, int min_len) {
    if (!m || pad_len < 0 || min_len < 0 || noise_len < 0) return MFB_ERR_ARG;
    const int need = pad_len > min_len ? pad_len : min_len;
    if (need > 0 && (!noise_iq || noise_len < need)) return MFB_ERR_ARG;
    if (noise_len > MOD_MAX_SAMPLES) return MFB_ERR_UNSUPPORTED;
    if (m->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->have = false;
    m->pad = m->min_len = m->noise_len = 0;
    if (need > 0) {
        HIPCHK(m->d_noise.alloc((size_t)need * sizeof(float2), hip_malloc));
        HIPCHK(hipMemcpy(m->d_noise, noise_iq, (size_t)need * sizeof(float2), hipMemcpyHostToDevice));
    }
    m->noise_len = need;
    m->pad = pad_len;
    m->min_len = min_len;
    return MFB_OK;
}

static void mod_launch_samples(mfb_modulator *m, const uint8_t *d_stage, mod_u64 *d_words) {
    const int B = m->B;
    const int64_t *d_soff = (const int64_t *)d_stage;
    const mod_u64 *d_d = (const mod_u64 *)(d_stage + (size_t)(B + 1) * 8);
    const int32_t *d_boff = (const int32_t *)(d_stage + (size_t)(B + 1) * 8 + (size_t)B * 16);
    hipLaunchKernelGGL(k_mod_samples, dim3((unsigned)((m->total + 255) / 256)), dim3(256), 0, m->stream, (const uint8_t *)m->d_rows,
                       (const mod_u64 *)m->d_symbase, d_boff, d_soff, B, (const mod_u64 *)m->d_P, d_d, m->sps, 1.0f / (float)m->sps, m->pad,
                       (const float2 *)m->d_noise, m->d_out.get(), d_words);
}

static int mod_begin_body(mfb_modulator *m, const uint8_t *bits, const int32_t *bit_off, const double *dphi_rad, int B) {
    const int nbits = bit_off[B], sps = m->sps, pad = m->pad;
    // the frames' places in the output
    m->sample_off.assign((size_t)B + 1, 0);
    int64_t total = 0;
    for (int f = 0; f < B; ++f) {
        int64_t len = (int64_t)(bit_off[f + 1] - bit_off[f]) * sps + 2 * (int64_t)pad;
        if (len < m->min_len) len = m->min_len;
        m->sample_off[f] = total;
        total += len;
    }
    m->sample_off[B] = total;
    if (total > MOD_MAX_SAMPLES) return MFB_ERR_UNSUPPORTED;
    if (total > m->max_samples) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(m->device));
    uint8_t *h = m->h_in;
    int64_t *h_soff = (int64_t *)h;
    mod_u64 *h_d = (mod_u64 *)(h + (size_t)(B + 1) * 8);
    mod_u64 *h_init = h_d + B;
    int32_t *h_boff = (int32_t *)(h_init + B);
    uint8_t *h_bits = (uint8_t *)(h_boff + B + 1);
    memcpy(h_soff, m->sample_off.data(), (size_t)(B + 1) * 8);
    for (int f = 0; f < B; ++f) {
        h_d[f] = dphi_rad ? mod_quantise(dphi_rad[f]) : 0;
        // FSK_LUT.py:31: - (2 b0 - 1) pi / 2, a quarter turn back for a leading 1 and forward for a leading 0
        h_init[f] = m->kind == MFB_MOD_FSK ? mod_quantise(bits[bit_off[f]] ? -1.5707963267948966 : 1.5707963267948966) : 0;
    }
    memcpy(h_boff, bit_off, (size_t)(B + 1) * 4);
    memcpy(h_bits, bits, (size_t)nbits);
    const size_t bytes = mod_staging_bytes(B, nbits);
    HIPCHK(hipMemcpyAsync(m->d_in, m->h_in, bytes, hipMemcpyHostToDevice, m->stream));
    const uint8_t *d = m->d_in;
    const mod_u64 *d_d = (const mod_u64 *)(d + (size_t)(B + 1) * 8);
    const mod_u64 *d_init = d_d + B;
    const int32_t *d_boff = (const int32_t *)(d_init + B);
    const uint8_t *d_bits = (const uint8_t *)(d_boff + B + 1);
    m->B = B;
    m->total = total;
    m->have = false;
    hipLaunchKernelGGL(k_mod_rows, dim3((nbits + 255) / 256), dim3(256), 0, m->stream, d_bits, d_boff, B, m->kind == MFB_MOD_GMSK3 ? 1 : 0,
                       m->d_rows.get());
    hipLaunchKernelGGL(k_mod_scan, dim3(B), dim3(MOD_THREADS), 0, m->stream, (const uint8_t *)m->d_rows, d_boff, (const mod_u64 *)m->d_T, d_d, d_init,
                       sps, m->d_symbase.get());
    mod_launch_samples(m, d, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->done, m->stream));
    m->busy = true;
    return MFB_OK;
}

extern "C" int mfb_modulator_begin(mfb_modulator *m, const uint8_t *bits, const int32_t *bit_off, const double *dphi_rad, int B) {
    if (!m || !bits || !bit_off || B < 1) return MFB_ERR_ARG;
    if (B > MOD_MAX_FRAMES) return MFB_ERR_UNSUPPORTED;
    if (bit_off[0] != 0) return MFB_ERR_ARG;
    if (m->busy || m->kind < 0) return MFB_ERR_STATE;
    const int min_bits = m->kind == MFB_MOD_GMSK3 ? 2 : 1;
    for (int f = 0; f < B; ++f) {
        const int64_t n = (int64_t)bit_off[f + 1] - bit_off[f];
        if (n < min_bits) return MFB_ERR_ARG;
        if (n > MOD_MAX_FRAME_BITS) return MFB_ERR_UNSUPPORTED;
        if (bit_off[f + 1] > m->max_bits) return MFB_ERR_ARG;
        if (dphi_rad && !std::isfinite(dphi_rad[f])) return MFB_ERR_ARG;
    }
    if (B > m->max_bits) return MFB_ERR_ARG;
    return guarded([&] { return mod_begin_body(m, bits, bit_off, dphi_rad, B); });
}

extern "C" int mfb_modulator_end(mfb_modulator *m, float *out_iq, int64_t *sample_off) {
    if (!m) return MFB_ERR_ARG;
    if (!m->busy) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(m->device));
    const int rc = m->finish(out_iq != nullptr, [&] {
        return hipMemcpyAsync(out_iq, m->d_out, (size_t)m->total * sizeof(float2), hipMemcpyDeviceToHost, m->stream);
    });
    if (rc) return rc;
    m->have = true;
    if (sample_off) memcpy(sample_off, m->sample_off.data(), (size_t)(m->B + 1) * sizeof(int64_t));
    return MFB_OK;
}

extern "C" int mfb_modulator_device_output(mfb_modulator *m, const void **dev_c64, int64_t *nsamples) {
    if (!m || !dev_c64) return MFB_ERR_ARG;
    if (m->busy || !m->have) return MFB_ERR_STATE;
    *dev_c64 = m->d_out.get();
    if (nsamples) *nsamples = m->total;
    return MFB_OK;
}

extern "C" int mfb_modulator_host_buffer(mfb_modulator *m, float **host_iq) {
    if (!m || !host_iq) return MFB_ERR_ARG;
    if (!m->h_out) {
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(m->h_out.alloc((size_t)m->max_samples * sizeof(float2), hip_host_malloc));
    }
    *host_iq = m->h_out;
    return MFB_OK;
}

extern "C" int mfb_debug_mod_phase(mfb_modulator *m, uint64_t *words, int64_t capacity) {
    if (!m || !words) return MFB_ERR_ARG;
    if (m->busy || !m->have) return MFB_ERR_STATE;
    if (capacity < m->total) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(m->device));
    DevBuf<mod_u64> d_words;
    HIPCHK(d_words.alloc((size_t)m->total * sizeof(mod_u64), hip_malloc));
    mod_launch_samples(m, m->d_in, d_words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(words, d_words, (size_t)m->total * sizeof(mod_u64), hipMemcpyDeviceToHost));
    return MFB_OK;
}
