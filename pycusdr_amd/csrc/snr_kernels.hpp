// The two means computeSNR takes over a block's spectrum windows (reference demodulator/demodulator_base.py:635-667, "DB:635-667"),
// on the device: np.mean(np.abs(window)) as float32, bit for bit as numpy computes it on the host, for a window of ANY length made of
// one or two pieces of the spectrum (piece 0 then piece 1: np.concatenate's order when the band wraps around 0 Hz).
//
//   |x|     clip_abs of clip_kernels.hpp (numpy's complex absolute value).
//   sum     np.add.reduce of float32: 8192-element chunks folded in order (s = chunk0; s = s + chunk1; ...); a chunk of n elements is
//           numpy's pairwise sum:
//             n < 8     a plain loop from 0;
//             n <= 128  eight strided accumulators seeded with the first eight elements, advanced over n - n % 8 elements, combined as
//                       ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 remaining elements one by one;
//             else      split at n2 = n / 2 - (n / 2) % 8 and add the two halves' sums.
//   mean    (float)((double)s / (double)n); NaN for an empty window, as np.mean of nothing.
//
// The recursion of a chunk is at most 7 splits deep (the longer half of n elements has at most n / 2 + 7.5: 8192 -> at most 79 after
// seven), so its nodes fit a binary heap of 255 slots: slot h at depth d = floor(log2(h + 1)) is reached from the root by the bits of
// h + 1 - 2^d.  Every thread finds its slot's (offset, length) by walking down; the leaves (at most 128, each at most 128 elements)
// are summed by eight lanes each, as clip_wave_sum does; the inner nodes are added level by level in LDS; one thread folds the chunk
// sums in order.  No atomics, a fixed order: the result does not depend on the grid.  No fast math, no contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "clip_kernels.hpp"

constexpr int SNR_THREADS = 256;
constexpr int SNR_CHUNK = 8192;      // numpy's reduction buffer, in elements
constexpr int SNR_LEAF = 128;        // numpy's pairwise leaf
constexpr int SNR_DEPTH = 7;         // splits below the root of a chunk, at most
constexpr int SNR_NODES = (2 << SNR_DEPTH) - 1;
constexpr int SNR_MAX_CHUNKS = (1 << 22) / SNR_CHUNK;      // chunks of the largest block

// element e of the window: piece 0, then piece 1
__device__ __forceinline__ float snr_elem(const float2 *X, int s0, int n0, int s1, int e) {
    return clip_abs(e < n0 ? X[s0 + e] : X[s1 + (e - n0)]);
}

// np.mean(np.abs(window)) of the window pieces[2][2] = [piece][start, length] of the spectrum X[N]; every thread of the workgroup
// (SNR_THREADS) calls it, thread 0 gets the mean.  A piece outside [0, N] (or N beyond the largest block) makes the window empty.
__device__ float band_mean_body(const float2 *X, int N, const int *pieces) {
#pragma clang fp contract(off)
    __shared__ int nlen[SNR_NODES], noff[SNR_NODES];      // per heap slot: 0 = no such node, -1 = inner node, else a leaf's length
    __shared__ float val[SNR_NODES];
    __shared__ float csum[SNR_MAX_CHUNKS];
    int s0 = pieces[0], n0 = pieces[1], s1 = pieces[2], n1 = pieces[3];
    if (s0 < 0 || n0 < 0 || s1 < 0 || n1 < 0 || n0 > N || n1 > N || s0 > N - n0 || s1 > N - n1 || n0 > N - n1 ||
        N > SNR_MAX_CHUNKS * SNR_CHUNK)
        n0 = n1 = 0;
    const int n = n0 + n1;
    if (n == 0) return NAN;
    const int nchunks = (n + SNR_CHUNK - 1) / SNR_CHUNK;
    const int tid = threadIdx.x, grp = tid >> 3, j = tid & 7;
    for (int c = 0; c < nchunks; ++c) {
        const int base = c * SNR_CHUNK, m = n - base < SNR_CHUNK ? n - base : SNR_CHUNK;
        // the recursion's nodes
        for (int h = tid; h < SNR_NODES; h += SNR_THREADS) {
            const int d = 31 - __clz(h + 1), k = h + 1 - (1 << d);
            int off = 0, len = m;
            for (int lv = d - 1; lv >= 0 && len > 0; --lv) {
                if (len <= SNR_LEAF) {
                    len = 0;       // an ancestor is a leaf
                } else {
                    const int n2 = len / 2 - (len / 2) % 8;
                    if ((k >> lv) & 1) {
                        off += n2;
                        len -= n2;
                    } else {
                        len = n2;
                    }
                }
            }
            noff[h] = off;
            nlen[h] = len > SNR_LEAF ? -1 : len;
        }
        __syncthreads();
        // the leaves: eight lanes each
        for (int h0 = 0; h0 < SNR_NODES; h0 += SNR_THREADS / 8) {
            const int h = h0 + grp;
            const int len = h < SNR_NODES ? nlen[h] : 0;
            const int off = base + (h < SNR_NODES ? noff[h] : 0);
            float acc = 0.f;
            const int body = len >= 8 ? len - len % 8 : 0;
            if (body > 0) {
                acc = snr_elem(X, s0, n0, s1, off + j);
                for (int i = 8; i < body; i += 8) acc = acc + snr_elem(X, s0, n0, s1, off + i + j);
            }
            acc = acc + __shfl_xor(acc, 1);
            acc = acc + __shfl_xor(acc, 2);
            acc = acc + __shfl_xor(acc, 4);
            if (j == 0 && len > 0) {
                for (int i = body; i < len; ++i) acc = acc + snr_elem(X, s0, n0, s1, off + i);
                val[h] = acc;
            }
        }
        __syncthreads();
        // the inner nodes, deepest first
        for (int d = SNR_DEPTH - 1; d >= 0; --d) {
            const int h = (1 << d) - 1 + tid;
            if (tid < (1 << d) && nlen[h] < 0) val[h] = val[2 * h + 1] + val[2 * h + 2];
            __syncthreads();
        }
        if (tid == 0) csum[c] = val[0];
        __syncthreads();
    }
    float mean = 0.f;
    if (tid == 0) {
        float s = csum[0];
        for (int c = 1; c < nchunks; ++c) s = s + csum[c];
        mean = (float)((double)s / (double)n);
    }
    return mean;
}

// One (block, window) per workgroup: grid (windows, blocks).  Block b's spectrum sits b * xstride elements on, the pieces of its
// window w at `pieces` + b * pstride bytes + w * 4 ints, its mean goes to `out` + b * ostride bytes + w floats.
//   behind k_pick_block:  pieces = &BlockScalars.band of the block's record, out = the first complex64 of its signal-window region
//                         ((mean_signal, mean_noise)), both strides the record's size;
//   mfb_debug_band_means: one window per "block" of the same injected spectrum (xstride 0).
__global__ void __launch_bounds__(SNR_THREADS) k_band_means(const float2 *X, size_t xstride, int N, const int *pieces, size_t pstride,
                                                            float *out, size_t ostride) {
    const size_t b = blockIdx.y;
    const int w = blockIdx.x;
    const int *p = reinterpret_cast<const int *>(reinterpret_cast<const uint8_t *>(pieces) + b * pstride) + 4 * w;
    const float mean = band_mean_body(X + b * xstride, N, p);
    if (threadIdx.x == 0) reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(out) + b * ostride)[w] = mean;
}
