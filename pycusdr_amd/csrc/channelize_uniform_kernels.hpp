// Uniform polyphase channeliser on the device (mfb_channelizer_create_uniform / _set_plan_uniform): one wideband capture -> the M
// channels of a raster, bin k centred on k fs / M, each low-pass filtered with the plan's real taps and decimated by D; the selected
// bins are written.  No reference counterpart: the reference takes one narrowband stream per radio process (pyCuSDR.py:245-251).
//
// Definition: the one of channelize_kernels.hpp with the exact words freq_k = k 2^64 / M (M a power of two).  Then
//     y_k[m] = sum_{t < T} h[t] x[m D - t] e^{-2 pi i k (m D - t) / M}                       x[n] = 0 for n < 0
//            = sum_{s < M} v_m[s] e^{+2 pi i k s / M}
//     u_m[p] = sum_{j : p + j M < T} h[p + j M] x[m D - p - j M]          p = 0 .. M - 1     (M branch sums, real taps)
//     v_m[s] = u_m[(s + m D) mod M]                                                          (a circular shift, no multiply)
// because e^{-2 pi i k (m D - p - j M) / M} = e^{+2 pi i k ((p - m D) mod M) / M}: one frame m costs T real-by-complex multiply-adds
// and one M-point transform, and yields every bin.
//
// Pure function of the absolute position.  u_m[p] is the work of one lane, which starts from (-0, -0) and adds its terms in the
// order j = 0, 1, ..., one fused multiply-add per component and tap, exactly the taps with p + j M < T (a branch without taps
// stays (-0, -0)).  The transform of a frame is chu_fft<M>: in-place decimation in frequency, passes of radix chu_radix(N) over
// sub-transforms of N = M, N / R, ... points, each butterfly the fixed sequence of additions of chu_dft4 / chu_dft8 followed by
// one multiplication with a table twiddle (two products and two fused multiply-adds; the outputs q = 0 and the last pass have
// none).  The table is e^{2 pi i q / M} rounded once from float64 on the host.  Radices, operands and order are a function of M
// alone: not of F, of the frame's slot in the workgroup, of the call's window or of the selected bins, which only choose what is
// read back out of the frame's image.  So a span computed in one call equals the same span computed in any number of calls, from
// any input window that covers it, with any selection, bit for bit.
// The outputs stay in the digit-reversed order the passes leave them in: bin k = q_1 + R_1 (q_2 + R_2 (q_3 ...)) stands in column
// q_1 M / R_1 + q_2 M / (R_1 R_2) + ... (chu_column); the store reads it there.
//
// Error bound, first order, per component, with u = 2^-24 and S_m = sum_t |h[t]| |x[m D - t]|.  A branch sum is a chain of
// J <= ceil(T / M) fused multiply-adds per component: its error is at most J u sum_j |h| |x| in modulus (the two components'
// term sums combine by the triangle inequality), J u S_m over all branches.  Every value inside the transform is a sum of branch
// sums times phasors, at most S_m in modulus over a frame's contributions.  A level of additions rounds by u relative; the
// (1 +- i) / sqrt(2) products inside chu_dft8 add one addition, one product and the constant's rounding, 3 u; a twiddle product
// with fused multiply-adds is within 2 u, its table entry within u: 3 u.  A radix-4 pass (2 bits of M): 2 + 3 = 5 u; a radix-8
// pass (3 bits): 3 + 3 + 3 = 9 u: at most 3 u per bit.  Errors pass on with gain 1.  Together
//     |device - model| <= (ceil(T / M) + 3 log2 M + 2) u S_m
// the 2 for the terms of second order.  The conversion of sc16 / sc8 is exact.
//
// Shape: a workgroup of 256 lanes makes F consecutive frames m0 .. m0 + F - 1 of all M bins.
//   stage   positions m0 D - (T - 1) .. (m0 + F - 1) D into LDS once, in natural order, converted as chz_load does; zeros below 0
//           and outside the call's input.
//   branch  lane tid owns branch p = tid mod M (256 is a multiple of M) of the frames tid / M + (256 / M) i: the tap h[p + j M] is
//           read once per j, coalesced along p, and serves four frames' chains.  Lanes along p read consecutive 8-byte words of the
//           span (descending): a ds_read_b64 of a 32-lane half touches each of the 64 banks once.  u goes into the frame's row of
//           the image already shifted, column (p - m D) mod M.
//   fft     the passes, a barrier between two.
//   store   lanes run along m: item (c, f) reads row f, column col[c] of the image and writes out[c][m0 + f - out_base], so one
//           store instruction covers consecutive outputs of a channel.  Rows are M + 1 float2 long: the stride of the transposed
//           read is 2 (M + 1) dwords, an odd multiple of 2, so 32 lanes of a ds_read_b64 fall on 32 different bank pairs.
// LDS: span + image + table <= CHU_LDS_BUDGET = 64 KiB, so two workgroups fit a CU's 160 KiB.  F = min(128, 4096 / M) where that
// fits, else the largest smaller multiple of max(16, 256 / M) that does, else 8 or 4 (M >= 128 with T + F D near 4096 only): F M is
// always a multiple of 256, and a channel's store is at least 128 contiguous bytes wherever F >= 16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channelize_kernels.hpp"
#include "channelize_plan.hpp"        // the CHU_ limits, chu_frames and chu_lds_bytes

typedef chz_cf chu_cf;

struct ChuPlan {                     // in device memory, written by mfb_channelizer_set_plan_uniform
    float2 tw[CHU_MAX_BINS];         // e^{2 pi i q / M}, q < M
    int32_t col[CHU_MAX_BINS];       // the image column of selected bin c
};

struct ChuArgs {
    int64_t in_base, in_end;         // the call's input holds the positions [in_base, in_end)
    int64_t out_base;
    int32_t out_count;
    int32_t D, T, F, nsel;
    int32_t out_stride;              // float2 between two selected bins' outputs
    float scale;
};

// the radix of the pass over sub-transforms of N points: 256 = 8 8 4, 128 = 8 4 4, 64 = 8 8, 32 = 8 4, 16 = 4 4, 8 = 8
__host__ __device__ constexpr int chu_radix(int N) { return (N >= 32 || N == 8) ? 8 : 4; }

// the image column in which the passes leave bin k
static inline int chu_column(int M, int k) {
    int col = 0;
    for (int N = M; N > 1;) {
        const int R = chu_radix(N), L = N / R;
        col += (k % R) * L;
        k /= R;
        N = L;
    }
    return col;
}

__host__ __device__ __forceinline__ chu_cf chu_add(chu_cf a, chu_cf b) { return (chu_cf){a.x + b.x, a.y + b.y}; }
__host__ __device__ __forceinline__ chu_cf chu_sub(chu_cf a, chu_cf b) { return (chu_cf){a.x - b.x, a.y - b.y}; }
__host__ __device__ __forceinline__ chu_cf chu_muli(chu_cf a) { return (chu_cf){-a.y, a.x}; }                     // i a
__host__ __device__ __forceinline__ chu_cf chu_mul(chu_cf a, chu_cf w) {
    return (chu_cf){fmaf(-a.y, w.y, a.x * w.x), fmaf(a.y, w.x, a.x * w.y)};
}

// a[q] <- sum_r a[r] e^{+2 pi i q r / 4}
__host__ __device__ __forceinline__ void chu_dft4(chu_cf &a0, chu_cf &a1, chu_cf &a2, chu_cf &a3) {
    const chu_cf t0 = chu_add(a0, a2), t1 = chu_sub(a0, a2), t2 = chu_add(a1, a3), t3 = chu_muli(chu_sub(a1, a3));
    a0 = chu_add(t0, t2);
    a1 = chu_add(t1, t3);
    a2 = chu_sub(t0, t2);
    a3 = chu_sub(t1, t3);
}

// a[q] <- sum_r a[r] e^{+2 pi i q r / 8}: the even and the odd inputs by chu_dft4, then a[q], a[q + 4] = E[q] +- w8^q O[q]
__host__ __device__ __forceinline__ void chu_dft8(chu_cf (&a)[8]) {
    const float c = 0.70710678118654752440f;
    chu_dft4(a[0], a[2], a[4], a[6]);
    chu_dft4(a[1], a[3], a[5], a[7]);
    const chu_cf o0 = a[1];
    const chu_cf o1 = (chu_cf){(a[3].x - a[3].y) * c, (a[3].x + a[3].y) * c};
    const chu_cf o2 = chu_muli(a[5]);
    const chu_cf o3 = (chu_cf){(-a[7].x - a[7].y) * c, (a[7].x - a[7].y) * c};
    const chu_cf e0 = a[0], e1 = a[2], e2 = a[4], e3 = a[6];
    a[0] = chu_add(e0, o0);
    a[1] = chu_add(e1, o1);
    a[2] = chu_add(e2, o2);
    a[3] = chu_add(e3, o3);
    a[4] = chu_sub(e0, o0);
    a[5] = chu_sub(e1, o1);
    a[6] = chu_sub(e2, o2);
    a[7] = chu_sub(e3, o3);
}

// One pass over the F frames of the image: the sub-transforms of N points become R = chu_radix(N) of N / R points each.
// Butterfly (sub-transform at `base`, i < L = N / R): a[r] = row[base + i + r L]; a <- DFT_R a; a[q] *= e^{2 pi i q i / N};
// row[base + i + q L] = a[q].
template <int M, int N>
__host__ __device__ __forceinline__ void chu_pass(chu_cf *img, const chu_cf *tw, int F, int tid) {
    constexpr int R = chu_radix(N), L = N / R, PER = M / R;
    for (int b = tid; b < F * PER; b += CHU_THREADS) {
        const int f = b / PER, w = b % PER;
        const int i = w % L;
        chu_cf *row = img + f * (M + 1) + (w / L) * N + i;
        chu_cf a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = row[r * L];
        if constexpr (R == 8) chu_dft8(a);
        else chu_dft4(a[0], a[1], a[2], a[3]);
        if constexpr (L > 1) {
#pragma unroll
            for (int q = 1; q < R; ++q) a[q] = chu_mul(a[q], tw[(q * i * (M / N)) & (M - 1)]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) row[q * L] = a[q];
    }
}

// the passes of every lane's share, a barrier between two
template <int M, int N = M>
__device__ __forceinline__ void chu_fft(chu_cf *img, const chu_cf *tw, int F, int tid) {
    chu_pass<M, N>(img, tw, F, tid);
    if constexpr (N / chu_radix(N) > 1) {
        __syncthreads();
        chu_fft<M, N / chu_radix(N)>(img, tw, F, tid);
    }
}

// Branch p of the NR frames f0, f0 + fstep, ...: the chains of u_m[p], stored shifted.  xs: the staged span, position
// m0 D - (T - 1) first; frame f, tap t reads xs[f D + T - 1 - t] with 0 <= f D <= f D + T - 1 - t <= (F - 1) D + T - 1.
template <int M, int NR>
__host__ __device__ __forceinline__ void chu_branch(const ChuArgs &A, const float *__restrict__ h, const chu_cf *xs, chu_cf *img, int64_t m0, int p,
                                                    int f0, int fstep) {
    chu_cf acc[NR];
    const chu_cf *x[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        acc[r] = (chu_cf){-0.0f, -0.0f};
        x[r] = xs + (f0 + r * fstep) * A.D + (A.T - 1);
    }
    for (int t = p; t < A.T; t += M) {
        const float g = h[t];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const chu_cf v = x[r][-t];
            acc[r].x = fmaf(g, v.x, acc[r].x);
            acc[r].y = fmaf(g, v.y, acc[r].y);
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int f = f0 + r * fstep;
        const int md = (int)(((uint64_t)(m0 + f) * (uint64_t)A.D) & (uint64_t)(M - 1));
        img[f * (M + 1) + ((p - md) & (M - 1))] = acc[r];
    }
}

// Grid: ceil(out_count / F) workgroups of CHU_THREADS lanes; dynamic LDS: chu_lds_bytes(M, D, T, F).  Every index is bounded: the
// input by in_base <= n < in_end, the span by p < (F - 1) D + T, the image by f < F and a column < M, the selection by c < nsel,
// the output by m < out_base + out_count.
template <int M, int FMT>
__global__ __launch_bounds__(CHU_THREADS) void k_chu(ChuArgs A, const ChuPlan *__restrict__ P, const void *__restrict__ raw,
                                                     const float *__restrict__ h, float2 *__restrict__ out) {
    extern __shared__ __align__(16) float2 chu_lds[];
    const int tid = threadIdx.x, F = A.F;
    const int span = (F - 1) * A.D + A.T;
    chu_cf *xs = (chu_cf *)chu_lds, *img = xs + span, *tw = img + F * (M + 1);
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
        const int p = tid % M, nf = F / FSTEP;                 // F M is a multiple of 256
        int i = 0;
        for (; i + 4 <= nf; i += 4) chu_branch<M, 4>(A, h, xs, img, m0, p, tid / M + i * FSTEP, FSTEP);
        for (; i < nf; ++i) chu_branch<M, 1>(A, h, xs, img, m0, p, tid / M + i * FSTEP, FSTEP);
    }
    __syncthreads();
    chu_fft<M>(img, tw, F, tid);
    __syncthreads();
    const int live = (int)((A.out_base + A.out_count - m0) < F ? (A.out_base + A.out_count - m0) : F);
    for (int b = tid; b < A.nsel * F; b += CHU_THREADS) {
        const int c = b / F, f = b - c * F;
        if (f >= live) continue;
        const chu_cf y = img[f * (M + 1) + P->col[c]];
        out[(size_t)c * A.out_stride + (size_t)(m0 - A.out_base) + f] = make_float2(y.x, y.y);
    }
}
