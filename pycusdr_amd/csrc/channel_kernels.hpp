// Radio channel on the device (mfb_channel_*): frames placed at their arrival times in one continuous stream, each on its own
// carrier that drifts linearly in frequency, white Gaussian noise underneath, optionally the grid of an ADC.  Restates awgn
// (examples/benchmark/create_signals.py:115-141) and the zero pad and mix of get_padded_packet (create_signals.py:197-198) of the
// reference, whose bench_modem.py builds its stream from N copies of one packet with fresh noise each.
//
// The stream is a pure function of (seed, frames, source, parameters, ABSOLUTE position n): nothing is carried from one sample to
// the next, so a span rendered in one call equals the same span rendered in any number of calls, under any grid, bit for bit.
//
//   out[n] = adc(gain_f * src[src_f + k] * e^{2 pi i phi_f(k) / 2^64} + sigma * (gI(n) + i gQ(n)))     k = n - start_f, f covers n
//   out[n] = adc(sigma * (gI(n) + i gQ(n)))                                                            no frame covers n
//   out[n] = +0 + 0i                                                                                   n < mute_before
//
// Phase: phi_f(k) = phase0 + k * freq + (k (k - 1) / 2) * rate, all uint64 in turns, wrapping modulo 2^64 -- the convention of
// mod_kernels.hpp; k < 2^31, so k (k - 1) / 2 < 2^61 is formed exactly before the wrapping product.  The word goes through
// mod_phase_to_iq; a word of 0 is (1, 0) and the sample is then not multiplied at all (select), so a frame with zero phase words
// and gain 1 passes its samples through bit for bit.  sigma == 0 adds nothing (uniform branch).
//
// Noise: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), key =
// the halves of the seed, counter = (low, high 32 bits of n >> 1, 0, 0).  Sample n takes words 2 (n & 1) and 2 (n & 1) + 1 of the
// block: one block serves the aligned pair (n & ~1, n | 1), which one thread renders and stores with 16 bytes (the first and the
// last sample of a window may be half a pair: one 8-byte store).  Box-Muller: the first word gives u = ((w >> 8) + 1) * 2^-24 in
// (0, 1], exact in fp32, and the radius sqrt(-2 ln u) -- at most sqrt(48 ln 2) = 5.77, the tail ends there; the second word, at
// the top of a uint64, is the angle's phase word through mod_phase_to_iq.  gI = r cos, gQ = r sin.
//
// ADC: q = rint(x / scale) (ties to even), saturated to the signed range of adc_bits, written as float(int(q)) * scale: exactly what
// k_unpack (unpack_kernels.hpp) computes from the integers a radio would have delivered.  scale is a power of two.
//
// Frames are sorted by start and do not overlap.  The frame that covers a sample is found as k_mod_samples finds it: a uniform
// bisection for the workgroup's first and last sample, per thread only where a frame starts inside the workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mod_kernels.hpp"

#define CHAN_THREADS 256             // a thread renders one aligned pair of samples

struct ChanFrame {                   // = mfb_channel_frame of mfbank.h, phases quantised
    int64_t start, src;
    int32_t length;
    float gain;
    mod_u64 phase0, freq, rate;
};

struct ChanArgs {
    int64_t base, mute_before;
    int32_t count, nframes;
    uint32_t key0, key1;
    float sigma;
    int32_t adc_bits;
    float adc_inv, adc_scale;        // 1 / scale and scale
};

__device__ inline void chan_philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
}

// Philox4x32-10 of counter (c0, c1, 0, 0)
__device__ inline void chan_philox(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t w[4]) {
    w[0] = c0;
    w[1] = c1;
    w[2] = 0;
    w[3] = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        chan_philox_round(w, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// two words -> (gI, gQ), standard normal each.  The radius is at most 5.77 (u >= 2^-24).
__device__ inline float2 chan_normals(uint32_t w0, uint32_t w1) {
    const float u = (float)((w0 >> 8) + 1u) * 0x1p-24f;
    const float r = __fsqrt_rn(-2.0f * logf(u));
    const float2 a = mod_phase_to_iq((mod_u64)w1 << 32);
    return make_float2(r * a.x, r * a.y);
}

// the last frame of [lo, hi) that starts at or before n; lo - 1 if none does
__device__ inline int chan_find(const ChanFrame *__restrict__ fr, int lo, int hi, int64_t n) {
    int a = lo - 1, b = hi;          // invariant: start[a] <= n < start[b], with the ends standing for -inf and +inf
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (fr[mid].start <= n) a = mid;
        else b = mid;
    }
    return a;
}

__device__ inline float chan_adc(float x, float inv, float scale, float lo, float hi) {
    float q = rintf(x * inv);
    q = q < lo ? lo : (q > hi ? hi : q);
    return (float)(int)q * scale;
}

// sample n, which frame f (or -1) may cover; w: the two Philox words of n
__device__ inline float2 chan_sample(const ChanArgs &A, const ChanFrame *__restrict__ fr, const float2 *__restrict__ src, int f, int64_t n,
                                     uint32_t w0, uint32_t w1) {
    if (n < A.mute_before) return make_float2(0.0f, 0.0f);
    float2 v = make_float2(0.0f, 0.0f);
    if (f >= 0) {
        const int64_t start = fr[f].start;
        const int64_t k = n - start;
        if (k >= 0 && k < (int64_t)fr[f].length) {        // (k < 0: the half pair in front of a window whose first sample starts a frame)
            const float2 s = src[fr[f].src + k];
            const mod_u64 uk = (mod_u64)k;
            const mod_u64 tri = (uk & 1) ? uk * ((uk - 1) >> 1) : (uk >> 1) * (uk - 1);      // k (k - 1) / 2, exact; 0 for k = 0
            const mod_u64 phi = fr[f].phase0 + uk * fr[f].freq + tri * fr[f].rate;
            float2 rot = s;
            if (phi != 0) {
                const float2 p = mod_phase_to_iq(phi);
                rot = make_float2(s.x * p.x - s.y * p.y, s.x * p.y + s.y * p.x);
            }
            const float g = fr[f].gain;
            v = make_float2(g * rot.x, g * rot.y);
        }
    }
    if (A.sigma != 0.0f) {
        const float2 g = chan_normals(w0, w1);
        v.x += A.sigma * g.x;
        v.y += A.sigma * g.y;
    }
    if (A.adc_bits) {
        const float hi = A.adc_bits == 8 ? 127.0f : 32767.0f, lo = -hi - 1.0f;
        v.x = chan_adc(v.x, A.adc_inv, A.adc_scale, lo, hi);
        v.y = chan_adc(v.y, A.adc_inv, A.adc_scale, lo, hi);
    }
    return v;
}

// out16 is 16-byte aligned and holds sample 2 (base >> 1) first: the window itself begins (base & 1) samples in.  Grid: one thread
// per aligned pair, ceil(pairs / CHAN_THREADS) workgroups; every index is bounded by base <= n < base + count.
__global__ __launch_bounds__(CHAN_THREADS) void k_chan_render(ChanArgs A, const ChanFrame *__restrict__ fr, const float2 *__restrict__ src,
                                                              float2 *__restrict__ out16) {
    const int64_t end = A.base + A.count;
    const int64_t pair0 = A.base >> 1;
    const int64_t gpair0 = pair0 + (int64_t)blockIdx.x * CHAN_THREADS;
    // the workgroup's first and last sample inside the window (uniform)
    const int64_t first = 2 * gpair0 > A.base ? 2 * gpair0 : A.base;
    int64_t last = 2 * gpair0 + 2 * CHAN_THREADS - 1;
    if (last > end - 1) last = end - 1;
    if (first > last) return;
    const int fa = A.nframes ? chan_find(fr, 0, A.nframes, first) : -1;
    const int fb = A.nframes ? chan_find(fr, fa < 0 ? 0 : fa, A.nframes, last) : -1;

    const int64_t pair = gpair0 + threadIdx.x;
    const int64_t n0 = 2 * pair, n1 = n0 + 1;
    const bool in0 = n0 >= A.base && n0 < end, in1 = n1 >= A.base && n1 < end;
    if (!in0 && !in1) return;
    int f0 = fa, f1 = fa;
    if (fb != fa) {                  // a frame starts inside the workgroup
        f0 = chan_find(fr, fa < 0 ? 0 : fa, fb + 1, n0);
        f1 = (f0 + 1 <= fb && fr[f0 + 1].start <= n1) ? f0 + 1 : f0;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    if (A.sigma != 0.0f) chan_philox((uint32_t)(mod_u64)pair, (uint32_t)((mod_u64)pair >> 32), A.key0, A.key1, w);
    // Both samples are always computed, by the one instruction sequence of their slot (a half pair computes its absent half from
    // valid operands and drops it): a sample's bits cannot depend on where a window's edge falls.
    const float2 a = chan_sample(A, fr, src, f0, n0, w[0], w[1]);
    const float2 b = chan_sample(A, fr, src, f1, n1, w[2], w[3]);
    float2 *o = out16 + (n0 - 2 * pair0);
    if (in0 && in1) *(float4 *)o = make_float4(a.x, a.y, b.x, b.y);
    else if (in0) o[0] = a;
    else o[1] = b;
}

// Test seam (mfb_debug_channel_normals): word pairs of the caller's choice through the production function.
__global__ __launch_bounds__(256) void k_chan_normals(const uint32_t *__restrict__ words, int npairs, float2 *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    out[i] = chan_normals(words[2 * i], words[2 * i + 1]);
}
