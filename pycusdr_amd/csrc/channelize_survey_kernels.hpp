// The survey of the raster (mfb_channelizer_set_survey / _survey_begin / _survey_end): per-bin power, noise floor and occupancy of
// the uniform channeliser's M bins, reduced from the workgroup's LDS image before -- or instead of -- the store.  No reference
// counterpart: the reference takes one narrowband stream per radio process (pyCuSDR.py:245-251).
//
// Definitions, with y_k[m] the uniform plan's output (channelize_uniform_kernels.hpp), bit for bit what k_chu makes:
//   cell    L = 2^l frames, 2 <= l <= 16; cell s of bin k covers the output positions [s L, (s + 1) L).
//   p_k[m]  = fl(fl(re re) + fl(im im)) in float32, not fused (chus_power forbids the contraction).
//   P[s][k] = the balanced pairwise sum of p_k[s L .. s L + L): at each level q[i] = fl(q[2 i] + q[2 i + 1]).  Every aligned
//             power-of-two run of frames is a subtree of it, so whoever holds such a run may sum it, and the order of the additions
//             does not depend on who did: not on the frames per workgroup, the grid, the cut of a span into calls, the input window,
//             the selected bins or whether outputs are written.  k runs in natural bin order.
//   floor[s] = the rank-th smallest (0-based) of P[s][0 .. M), an exact selection.
//   mask     bit (s, k) is set iff P[s][k] > fl(threshold floor[s]); uint32 mask[s][ceil(M / 32)], bit j of word w is bin 32 w + j,
//            unused bits zero.
//
// Shape.  k_chus<M, FMT, WRITE> is k_chu with a power-of-two frame count Fs = chus_frames (the largest power of two that is at most
// the plan's F and fits the same LDS budget with the 1 KiB of scratch below) and one more phase behind chu_fft: staging, chu_branch,
// chu_pass and chu_fft are the uniform kernel's own, so the image holds the same bits, and WRITE stores the selected bins as k_chu
// does.  A survey call's out_base and out_count are multiples of L and workgroup b starts at out_base + b Fs, so with the chunk
// C = min(L, Fs) every workgroup holds Fs / C aligned chunks, each a whole cell (L <= Fs) or a subtree of one (L > Fs).
//   reduce   lane tid reads column tid mod M of the R = Fs M / 256 consecutive rows from (tid / M) R on: lanes run along columns, rows
//            are M + 1 float2 long, so a wave's ds_read_b64 covers consecutive words.  It sums them as subtrees of S = min(R, C) frames
//            in registers (chus_tree).  Where C <= R these are whole chunks and go to device memory; otherwise one value per lane goes
//            to the 256-float scratch, and behind a barrier lane (j, col) of the first (Fs / C) M takes the C / R values of its chunk up
//            the remaining levels.
//   write    part[chunk][bin], chunk counted from out_base in units of C, bin = chus_bin(col), the inverse of chu_column.
// k_chus_finish, one workgroup of 256 lanes per cell, takes the n = L / C partials of every bin up the remaining levels -- the lanes
// of group tid / M sum an aligned run of n / G partials each (G = min(256 / M, n)) with the binary-counter form of the same tree,
// lane (0, k) sums the G results --, selects the floor by counting, for every bin, the values below it (ties broken by the index: the
// ranks are a permutation, exactly one lane holds `rank`; the comparison is on the bit patterns, which order non-negative floats as
// the floats themselves), and packs the mask words.  No atomics; nothing depends on the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channelize_plan.hpp"        // the CHUS_ limits, chus_frames and chus_lds_bytes
#include "channelize_uniform_kernels.hpp"

struct ChusArgs {
    int32_t L;                       // frames per cell
    int32_t C;                       // frames per partial: min(L, Fs)
    int32_t M, rank;
    float threshold;
};

// the bin that the passes leave in image column col: the inverse of chu_column
template <int M>
__host__ __device__ __forceinline__ int chus_bin(int col) {
    int k = 0, mul = 1;
#pragma unroll
    for (int N = M; N > 1;) {
        const int R = chu_radix(N), Lq = N / R;
        k += (col / Lq) * mul;
        col %= Lq;
        mul *= R;
        N = Lq;
    }
    return k;
}

// Contraction is switched off by pragma: HIP's __fmul_rn / __fadd_rn are plain `x * y` / `x + y` in the headers, and under the
// compiler's default -ffp-contract=fast-honor-pragmas they would fuse after inlining (re re + im im into one v_fma_f32, one
// rounding fewer than the definition).  The operators below carry no contract flag, so no product can be fused into these sums.
__host__ __device__ __forceinline__ float chus_power(chu_cf y) {
#pragma clang fp contract(off)
    const float a = y.x * y.x;
    const float b = y.y * y.y;
    return a + b;
}

__host__ __device__ __forceinline__ float chus_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__host__ __device__ __forceinline__ float chus_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// the subtree of N frames (rows `stride` float2 apart) of one column
template <int N>
__host__ __device__ __forceinline__ float chus_tree(const chu_cf *p, int stride) {
    if constexpr (N == 1) return chus_power(p[0]);
    else return chus_add(chus_tree<N / 2>(p, stride), chus_tree<N / 2>(p + (N / 2) * stride, stride));
}

// the tree over n = 2^j values v[0], v[step], ...: a binary counter, the pending left operands of every level in st[level * 256]
__device__ __forceinline__ float chus_run(const float *v, size_t step, int n, float *st) {
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) {
        acc = v[(size_t)i * step];
        int lvl = 0;
        for (int t = i; t & 1; t >>= 1, ++lvl) acc = chus_add(st[lvl * 256], acc);
        st[lvl * 256] = acc;
    }
    return acc;
}

// The reduce and write phases of the header, behind a barrier that follows chu_fft.  sc: CHUS_SCRATCH floats.  live: the frames of
// this workgroup inside the call, a multiple of C.  part: the partials of chunk 0 of this workgroup.
template <int M>
__device__ __forceinline__ void chus_reduce(const chu_cf *img, float *sc, int F, int C, int live, float *__restrict__ part, int tid) {
    constexpr int G = CHU_THREADS / M;
    const int R = F / G;                                   // F M is a multiple of 256; R is a power of two, at most 16
    const int col = tid % M, g = tid / M;
    const int S = R < C ? R : C;
    const chu_cf *p = img + (g * R) * (M + 1) + col;
    const int bin = chus_bin<M>(col);
    for (int i = 0; i < R; i += S) {
        float v;
        switch (S) {
            case 1: v = chus_tree<1>(p + i * (M + 1), M + 1); break;
            case 2: v = chus_tree<2>(p + i * (M + 1), M + 1); break;
            case 4: v = chus_tree<4>(p + i * (M + 1), M + 1); break;
            case 8: v = chus_tree<8>(p + i * (M + 1), M + 1); break;
            default: v = chus_tree<16>(p + i * (M + 1), M + 1); break;
        }
        if (C <= R) {
            const int f = g * R + i;                       // the chunk's first frame
            if (f < live) part[(size_t)(f / C) * M + bin] = v;
        } else {
            sc[tid] = v;
        }
    }
    if (C > R) {                                           // (uniform over the workgroup)
        __syncthreads();
        const int n = C / R;                               // lane values per chunk, 2 .. G
        if (tid < (F / C) * M) {
            const int j = tid / M;
            if (j * C < live) {
                const float *v = sc + (j * n) * M + col;
                float q[G > 1 ? G : 1];
#pragma unroll
                for (int i = 0; i < G; ++i) q[i] = i < n ? v[i * M] : 0.0f;
#pragma unroll
                for (int w = 1; w < G; w <<= 1) {
#pragma unroll
                    for (int i = 0; i + w < G; i += 2 * w)
                        if (i + w < n) q[i] = chus_add(q[i], q[i + w]);
                }
                part[(size_t)j * M + bin] = q[0];
            }
        }
    }
}

// Grid: out_count / Fs workgroups, rounded up, of CHU_THREADS lanes; dynamic LDS: chus_lds_bytes(M, D, T, Fs).  A.F = Fs.  The bounds of
// k_chu hold as they are; a partial's index is below out_count / C because its chunk begins inside the call (f < live) and out_count
// is a multiple of C.
template <int M, int FMT, bool WRITE>
__global__ __launch_bounds__(CHU_THREADS) void k_chus(ChuArgs A, ChusArgs V, const ChuPlan *__restrict__ P, const void *__restrict__ raw,
                                                      const float *__restrict__ h, float2 *__restrict__ out, float *__restrict__ part) {
    extern __shared__ __align__(16) float2 chu_lds[];
    const int tid = threadIdx.x, F = A.F;
    const int span = (F - 1) * A.D + A.T;
    chu_cf *xs = (chu_cf *)chu_lds, *img = xs + span, *tw = img + F * (M + 1);
    float *sc = (float *)(tw + M);
    const int64_t m0 = A.out_base + (int64_t)blockIdx.x * F;
    const int64_t n0 = m0 * A.D - (A.T - 1);
    for (int p = tid; p < span; p += CHU_THREADS) {
        const int64_t n = n0 + p;
        float2 v = make_float2(0.0f, 0.0f);
        if (n >= A.in_base && n < A.in_end) v = chz_load<FMT>(raw, n - A.in_base, A.scale);
        xs[p] = (chu_cf){v.x, v.y};
    }
    if (tid < M) tw[tid] = (chu_cf){P->tw[tid].x, P->tw[tid].y};
    __syncthreads();
    {
        constexpr int FSTEP = CHU_THREADS / M;
        const int p = tid % M, nf = F / FSTEP;
        int i = 0;
        for (; i + 4 <= nf; i += 4) chu_branch<M, 4>(A, h, xs, img, m0, p, tid / M + i * FSTEP, FSTEP);
        for (; i < nf; ++i) chu_branch<M, 1>(A, h, xs, img, m0, p, tid / M + i * FSTEP, FSTEP);
    }
    __syncthreads();
    chu_fft<M>(img, tw, F, tid);
    __syncthreads();
    const int live = (int)((A.out_base + A.out_count - m0) < F ? (A.out_base + A.out_count - m0) : F);
    chus_reduce<M>(img, sc, F, V.C, live, part + (size_t)((m0 - A.out_base) / V.C) * M, tid);
    if constexpr (WRITE) {
        for (int b = tid; b < A.nsel * F; b += CHU_THREADS) {
            const int c = b / F, f = b - c * F;
            if (f >= live) continue;
            const chu_cf y = img[f * (M + 1) + P->col[c]];
            out[(size_t)c * A.out_stride + (size_t)(m0 - A.out_base) + f] = make_float2(y.x, y.y);
        }
    }
}

// Grid: one workgroup of 256 lanes per cell.  part: [ncells L / C][M]; power [ncells][M], floor [ncells], mask [ncells][ceil(M / 32)].
__global__ __launch_bounds__(256) void k_chus_finish(ChusArgs V, const float *__restrict__ part, float *__restrict__ power,
                                                     float *__restrict__ floor_, uint32_t *__restrict__ mask) {
    __shared__ float st[(CHUS_MAX_LOG2 + 1) * 256];        // the counters' pending operands, a column per lane
    __shared__ float sg[256];
    __shared__ float sp[CHU_MAX_BINS];
    __shared__ float lev;
    const int tid = threadIdx.x, M = V.M, k = tid % M, g = tid / M;
    const int n = V.L / V.C;                               // partials per (cell, bin): a power of two
    const int G = 256 / M < n ? 256 / M : n;               // lane groups at work
    const int per = n / G;
    const float *cell = part + (size_t)blockIdx.x * n * M;
    if (g < G) sg[tid] = chus_run(cell + (size_t)g * per * M + k, (size_t)M, per, st + tid);
    __syncthreads();
    if (tid < M) sp[tid] = chus_run(sg + tid, (size_t)M, G, st + tid);
    __syncthreads();
    if (tid < M) {
        const float mine = sp[tid];
        const uint32_t key = __float_as_uint(mine);
        int below = 0;
        for (int j = 0; j < M; ++j) {
            const uint32_t o = __float_as_uint(sp[j]);
            below += (o < key || (o == key && j < tid)) ? 1 : 0;
        }
        power[(size_t)blockIdx.x * M + tid] = mine;
        if (below == V.rank) {
            floor_[blockIdx.x] = mine;
            lev = chus_mul(V.threshold, mine);
        }
    }
    __syncthreads();
    const int words = (M + 31) / 32;
    if (tid < words) {
        uint32_t w = 0;
        for (int j = 0; j < 32; ++j) {
            const int b = 32 * tid + j;
            if (b < M && sp[b] > lev) w |= 1u << j;
        }
        mask[(size_t)blockIdx.x * words + tid] = w;
    }
}
