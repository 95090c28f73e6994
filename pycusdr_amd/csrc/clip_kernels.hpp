// Interference-peak clipping of a block (or of the blocks of a batch) on the device, before the forward transform: the
// reference's __thresholdInput (demodulator/demodulator_base.py:670-707, "DB:670-707"), bit for bit as numpy computes it on
// the host -- the clipped samples and the ascending indices of the second round (clippedPeakIPure).
//
//   |x|     numpy's complex absolute value: L = max(|re|, |im|), S = min, |x| = L * sqrt(fma(S/L, S/L, 1)); 0 for L == 0,
//           inf when either part is inf, NaN when either is NaN.
//   mean    np.mean of float32: 8192-element chunks folded in order (s = s + chunk); a chunk is numpy's pairwise sum -- for
//           the power-of-two blocks used here a balanced tree of 128-element leaves, each leaf eight strided accumulators
//           r[j] += v[i + j] combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).  mean = (float)((double)s / N).
//   clip    t = (float)scale * mean; |x| > t:  x <- t * (x / |x|) in numpy's complex arithmetic (divide by a real:
//           (re + im * 0) * (1 / |x|), (im - re * 0) * (1 / |x|); multiply by t + 0j).
//   twice   round 2 recomputes |x| of the clipped samples only, sums again, clips above the new threshold; its indices are
//           the result.
//
// Work unit: a wave and 1024 consecutive samples (8 leaves).  The four kernels of a batch run every (block, wave) at once
// with each block's overlap as it sits in the window (block 0: the chain tail of the previous call); k_clip_chain then
// redoes, in order, the blocks whose predecessor changed a sample of its last `ov` samples -- the only case in which a block's
// real overlap (the previous block's clipped tail, reference demodulator_process.py:293,337) differs from the window's.
// Compaction: per-wave counts and a scan, no atomics.  No fast math, no contraction (`fp contract(off)` in every function that
// computes), correctly rounded division and square root (plain `/` and __builtin_sqrtf: HIP's __fsqrt_rn is the native
// approximation unless OCML's rounded operations are enabled).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr int CLIP_WAVE = 1024;      // samples per wave
constexpr int CLIP_LEAF = 128;       // numpy's pairwise leaf
constexpr int CLIP_CHUNK_LEAVES = 64; // 8192-element reduction buffer
constexpr int CLIP_THREADS = 256;    // parallel kernels: four waves per workgroup
constexpr int CLIP_CHAIN_THREADS = 1024;
constexpr int CLIP_MAX_CHUNKS = (1 << 22) / (CLIP_LEAF * CLIP_CHUNK_LEAVES);   // 8192-element chunks of the largest block
constexpr int CLIP_HEAD = 256;       // per block: int32 count, then the first CLIP_HEAD - 1 indices (read back with the record)

struct ClipTail {                    // the previous block's clipped last `ov` samples (chain across calls)
    int32_t valid, pad[3];
    float2 s[1];
};

struct ClipArgs {
    const float2 *x;                 // raw samples: block b at x + b * xstride
    long long xstride;
    float2 *y;                       // clipped blocks [nb][N]
    int32_t *idx;                    // indices [nb][N]
    int32_t *head;                   // [nb][CLIP_HEAD]
    float *s1, *s2;                  // leaf sums [nb][N / 128] of the two rounds
    float *thr;                      // [nb][2]
    int32_t *wcnt, *wflag;           // [nb][N / 1024]: indices per wave, wave changed a sample of the block's tail
    ClipTail *tail;                  // nullptr: no chain (ov == 0)
    int N, ov, nb;
    float scale;
};

__device__ __forceinline__ float clip_abs(float2 v) {
#pragma clang fp contract(off)
    const float a = fabsf(v.x), b = fabsf(v.y);
    if (isinf(a) || isinf(b)) return INFINITY;
    if (isnan(a) || isnan(b)) return NAN;
    const float L = fmaxf(a, b), S = fminf(a, b);
    if (L == 0.f) return 0.f;
    const float r = S / L;
    return __builtin_sqrtf(fmaf(r, r, 1.0f)) * L;
}
__device__ __forceinline__ float2 clip_scale(float2 v, float m, float t) {
#pragma clang fp contract(off)
    const float inv = 1.0f / m;
    const float qr = (v.x + v.y * 0.f) * inv, qi = (v.y - v.x * 0.f) * inv;
    return make_float2(t * qr - 0.f * qi, t * qi + 0.f * qr);
}
// sample i of block b as this pass sees it: the first ov from `prev` (the previous block's clipped tail) when given
__device__ __forceinline__ float2 clip_in(const ClipArgs &a, int b, const float2 *prev, int i) {
    return (prev && i < a.ov) ? prev[i] : a.x[(long long)b * a.xstride + i];
}
// |x| after round 1 (t1 < 0: round 1 not applied yet) and the round-1 sample
__device__ __forceinline__ float clip_mag2(float2 &v, float t1) {
    float m = clip_abs(v);
    if (t1 >= 0.f && m > t1) {
        v = clip_scale(v, m, t1);
        m = clip_abs(v);
    }
    return m;
}
__device__ __forceinline__ const float2 *clip_prev0(const ClipArgs &a) {
    return (a.tail && a.tail->valid) ? a.tail->s : nullptr;
}

// leaf sums of one wave's 1024 samples: lane = 8 * leaf + j
__device__ void clip_wave_sum(const ClipArgs &a, int b, const float2 *prev, int w, float t1, float *S) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, leaf = lane >> 3, j = lane & 7;
    const int base = w * CLIP_WAVE + leaf * CLIP_LEAF + j;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float2 v = clip_in(a, b, prev, base + 8 * i);
        const float m = clip_mag2(v, t1);
        acc = i ? acc + m : m;
    }
    acc = acc + __shfl_xor(acc, 1);
    acc = acc + __shfl_xor(acc, 2);
    acc = acc + __shfl_xor(acc, 4);
    if (j == 0) S[(size_t)b * (a.N / CLIP_LEAF) + w * 8 + leaf] = acc;
}

// (float)scale * np.mean from the leaf sums of block b; every thread of the workgroup calls it, all get the threshold
__device__ float clip_threshold(const ClipArgs &a, const float *S, int b, float *lds) {
#pragma clang fp contract(off)
    const int nleaves = a.N / CLIP_LEAF;
    const int cl = nleaves < CLIP_CHUNK_LEAVES ? nleaves : CLIP_CHUNK_LEAVES;
    const int nchunks = nleaves / cl;
    const float *Sb = S + (size_t)b * nleaves;
    for (int k = threadIdx.x; k < nchunks; k += blockDim.x) {
        float r[CLIP_CHUNK_LEAVES];
#pragma unroll
        for (int i = 0; i < CLIP_CHUNK_LEAVES; ++i) r[i] = i < cl ? Sb[k * cl + i] : 0.f;
#pragma unroll
        for (int w = 1; w < CLIP_CHUNK_LEAVES; w *= 2) {
            if (w < cl) {
#pragma unroll
                for (int i = 0; i < CLIP_CHUNK_LEAVES; i += 2 * w) r[i] = r[i] + r[i + w];
            }
        }
        lds[k] = r[0];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int k = 0; k < nchunks; ++k) s = s + lds[k];
        const float mean = (float)((double)s / (double)a.N);
        lds[nchunks] = a.scale * mean;
    }
    __syncthreads();
    const float t = lds[nchunks];
    __syncthreads();
    return t;
}

// final samples of one wave (lane-strided), their index count and whether the block's tail changed
__device__ void clip_wave_apply(const ClipArgs &a, int b, const float2 *prev, int w, float t1, float t2) {
    const int lane = threadIdx.x & 63;
    int cnt = 0, changed = 0;
    float2 *yb = a.y + (size_t)b * a.N;
    const float2 *raw = a.x + (long long)b * a.xstride;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int i = w * CLIP_WAVE + k * 64 + lane;
        float2 v = clip_in(a, b, prev, i);
        const float m = clip_mag2(v, t1);
        if (m > t2) {
            v = clip_scale(v, m, t2);
            ++cnt;
        }
        yb[i] = v;
        if (i >= a.N - a.ov) {
            const float2 r = raw[i];
            changed |= (int)(__float_as_uint(r.x) != __float_as_uint(v.x)) | (int)(__float_as_uint(r.y) != __float_as_uint(v.y));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        changed |= __shfl_xor(changed, o);
    }
    if (lane == 0) {
        a.wcnt[(size_t)b * (a.N / CLIP_WAVE) + w] = cnt;
        a.wflag[(size_t)b * (a.N / CLIP_WAVE) + w] = changed;
    }
}

// ascending indices of one wave: lane takes 16 consecutive samples, the wave scans, earlier waves' counts give the base
__device__ void clip_wave_compact(const ClipArgs &a, int b, const float2 *prev, int w, float t1, float t2) {
    const int lane = threadIdx.x & 63;
    const int nw = a.N / CLIP_WAVE;
    const int32_t *cb = a.wcnt + (size_t)b * nw;
    int base = 0, total = 0;
    for (int q = lane; q < nw; q += 64) {
        const int n = cb[q];
        base += q < w ? n : 0;
        total += n;
    }
    for (int o = 32; o > 0; o >>= 1) {
        base += __shfl_xor(base, o);
        total += __shfl_xor(total, o);
    }
    unsigned mask = 0;
    const int i0 = w * CLIP_WAVE + lane * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float2 v = clip_in(a, b, prev, i0 + k);
        const float m = clip_mag2(v, t1);
        mask |= (m > t2 ? 1u : 0u) << k;
    }
    const int mine = __popc(mask);
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    int pos = base + incl - mine;
    int32_t *ib = a.idx + (size_t)b * a.N;
    int32_t *hb = a.head + (size_t)b * CLIP_HEAD;
    while (mask) {
        const int k = __ffs(mask) - 1;
        mask &= mask - 1;
        ib[pos] = i0 + k;
        if (pos < CLIP_HEAD - 1) hb[1 + pos] = i0 + k;
        ++pos;
    }
    if (w == 0 && lane == 0) hb[0] = total;
}

// ---- the parallel pass: grid (N / 4096, nb), CLIP_THREADS ------------------------------------------------------------------
__global__ void __launch_bounds__(CLIP_THREADS) k_clip_sum1(ClipArgs a) {
    const int b = blockIdx.y, w = blockIdx.x * (CLIP_THREADS / 64) + (threadIdx.x >> 6);
    clip_wave_sum(a, b, b == 0 ? clip_prev0(a) : nullptr, w, -1.f, a.s1);
}
__global__ void __launch_bounds__(CLIP_THREADS) k_clip_sum2(ClipArgs a) {
    __shared__ float lds[CLIP_MAX_CHUNKS + 1];
    const int b = blockIdx.y, w = blockIdx.x * (CLIP_THREADS / 64) + (threadIdx.x >> 6);
    const float t1 = clip_threshold(a, a.s1, b, lds);
    clip_wave_sum(a, b, b == 0 ? clip_prev0(a) : nullptr, w, t1, a.s2);
}
__global__ void __launch_bounds__(CLIP_THREADS) k_clip_apply(ClipArgs a) {
    __shared__ float lds[CLIP_MAX_CHUNKS + 1];
    const int b = blockIdx.y, w = blockIdx.x * (CLIP_THREADS / 64) + (threadIdx.x >> 6);
    const float t1 = clip_threshold(a, a.s1, b, lds);
    const float t2 = clip_threshold(a, a.s2, b, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.thr[2 * b] = t1;
        a.thr[2 * b + 1] = t2;
    }
    clip_wave_apply(a, b, b == 0 ? clip_prev0(a) : nullptr, w, t1, t2);
}
__global__ void __launch_bounds__(CLIP_THREADS) k_clip_compact(ClipArgs a) {
    const int b = blockIdx.y, w = blockIdx.x * (CLIP_THREADS / 64) + (threadIdx.x >> 6);
    clip_wave_compact(a, b, b == 0 ? clip_prev0(a) : nullptr, w, a.thr[2 * b], a.thr[2 * b + 1]);
}

// ---- the chain: one workgroup, blocks in order -------------------------------------------------------------------------------
// Block b (b >= 1) is redone from its real overlap -- block b - 1's clipped tail -- when block b - 1 changed any of its last
// ov samples; then the last block's tail is kept for the next call.
__global__ void __launch_bounds__(CLIP_CHAIN_THREADS) k_clip_chain(ClipArgs a) {
    __shared__ float lds[CLIP_MAX_CHUNKS + 1];
    __shared__ int redo;
    const int nw = a.N / CLIP_WAVE, wave = threadIdx.x >> 6, waves = CLIP_CHAIN_THREADS / 64;
    const int wfirst = (a.N - a.ov) / CLIP_WAVE;
    for (int b = 1; b < a.nb; ++b) {
        if (threadIdx.x == 0) {
            int r = 0;
            for (int w = wfirst; w < nw; ++w) r |= a.wflag[(size_t)(b - 1) * nw + w];
            redo = r;
        }
        __syncthreads();
        const bool again = redo != 0;
        __syncthreads();
        if (!again) continue;
        const float2 *prev = a.y + (size_t)(b - 1) * a.N + (a.N - a.ov);
        for (int w = wave; w < nw; w += waves) clip_wave_sum(a, b, prev, w, -1.f, a.s1);
        __threadfence();
        __syncthreads();
        const float t1 = clip_threshold(a, a.s1, b, lds);
        for (int w = wave; w < nw; w += waves) clip_wave_sum(a, b, prev, w, t1, a.s2);
        __threadfence();
        __syncthreads();
        const float t2 = clip_threshold(a, a.s2, b, lds);
        for (int w = wave; w < nw; w += waves) clip_wave_apply(a, b, prev, w, t1, t2);
        __threadfence();
        __syncthreads();
        for (int w = wave; w < nw; w += waves) clip_wave_compact(a, b, prev, w, t1, t2);
        __threadfence();
        __syncthreads();
    }
    if (a.tail) {
        const float2 *last = a.y + (size_t)(a.nb - 1) * a.N + (a.N - a.ov);
        for (int i = threadIdx.x; i < a.ov; i += blockDim.x) a.tail->s[i] = last[i];
        if (threadIdx.x == 0) a.tail->valid = 1;
    }
}
