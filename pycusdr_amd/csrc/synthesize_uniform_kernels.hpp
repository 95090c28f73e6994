// Uniform polyphase synthesiser on the device (mfb_synthesizer_*): narrowband streams -> one wideband stream, stream b centred on
// bin b of an M-bin raster, each zero-stuffed by I, low-pass filtered with the plan's real taps and mixed to b fs / M; the streams
// are summed.  The dual of k_chu (channelize_uniform_kernels.hpp), whose chu_* helpers it uses unchanged.  No reference
// counterpart: the reference makes one narrowband stream per radio process (pyCuSDR.py:245-251).
//
// Definition.  x_b[m], m >= 0, is the narrow stream of bin b: fl(gain source[src + m - start]) (float32, one rounding per component;
// a gain of 1 multiplies nothing) where a placement (bin, start, src, length, gain) covers m, 0 elsewhere; placements of one bin do
// not overlap.  With n the absolute wide position, (q, r) = divmod(n, I) and the exact words freq_b = b 2^64 / M:
//     w[n] = sum_b e^{+2 pi i b n / M} sum_{j >= 0 : r + j I < T} h[r + j I] x_b[q - j]
//          = sum_{j >= 0 : r + j I < T} h[r + j I] X_{q - j}[n mod M]
//     X_m[s] = sum_b x_b[m] e^{+2 pi i b s / M}                                              s = 0 .. M - 1
// because e^{2 pi i b n / M} depends on n mod M alone: one input frame m costs one M-point transform, whatever the number of
// occupied bins, and one output ceil((T - r) / I) real-by-complex multiply-adds.
//
// Pure function of the absolute position.  A frame's image row holds x_b[m] in column b, natural bin order, and +0 in the columns
// of bins without a sample; chu_fft<M> transforms it in place -- radices, operands and order a function of M alone, see
// channelize_uniform_kernels.hpp -- and leaves X_m[s] in column chu_column(M, s).  w[n] is the work of one lane, which starts from
// (-0, -0) and adds its terms in the order j = 0, 1, ..., one fused multiply-add per component and tap, exactly the taps with
// r + j I < T.  Nothing depends on F, on the frame's row in the workgroup, on the call's span or on the output set: a span computed
// in one call equals the same span computed in any number of calls, bit for bit.
//
// Positions are int64: q0 = out_base div I + F blockIdx, the first frame m_lo = q0 - (J - 1) of the image, n, n mod M and
// m - start are 64-bit; what is narrowed to int is an offset inside the workgroup's tile, n - m_lo I < R I <= 2^18.
//
// Error bound, first order, per component, with u = 2^-24 and S[n] = sum_j |h[r + j I]| sum_b |x_b[q - j]|.  The gain's product
// rounds x_b by u.  Every value inside the transform of frame m is a sum of the x_b[m] times phasors, at most sum_b |x_b[m]| in
// modulus; the passes cost at most 3 u per bit of M (channelize_uniform_kernels.hpp: 5 u per radix-4 pass, 9 u per radix-8 pass),
// errors passing on with gain 1: |X^_m[s] - X_m[s]| <= (1 + 3 log2 M) u sum_b |x_b[m]|.  The output is a chain of at most
// J = ceil(T / I) fused multiply-adds per component, whose first has the exact addend -0: term j is rounded at most J times,
// J u sum_j |h| |X|.  Together
//     |device - model| <= (ceil(T / I) + 3 log2 M + 3) u S[n]
// the last 2 for the terms of second order.
//
// Shape: a workgroup of 256 lanes makes the F I consecutive outputs q0 I .. (q0 + F) I - 1 of the F frames q0 .. q0 + F - 1, cut to
// the call's span, from the R = F + J - 1 input frames m_lo .. q0 + F - 1 that they read.  Frames below 0 hold zeros.
//   clear   the image, R rows of M + 1 float2: consecutive words, every bank once per 32 lanes.  The twiddle table and the taps go
//           into LDS beside it.
//   place   every occupied bin has G lanes of its own, G the largest power of two with G nocc <= 256.  They find the bin's first
//           placement that can meet the frames m_lo .. m_lo + R - 1 (a binary search in that bin's placements, sorted by start
//           on the host) -- every lane reads the descriptors once, all bins at the same time, so a workgroup waits for one
//           chain of loads whatever the number of bins -- and walk the placements that do; of each, lane `sub` stores the
//           samples of the rows r0 + sub, r0 + sub + G, ..., times the gain, into (row, column bin): G consecutive source samples
//           per load, loads that do not depend on one another.  Within a bin the store's stride is 2 (M + 1) dwords, an odd
//           multiple of 2: up to 32 lanes of a ds_write_b64 fall on different bank pairs.  Where G < 32 a half-wave holds 32 / G
//           bins, and (row, bin) and (row', bin') meet where row (M + 1) + bin = row' (M + 1) + bin' modulo 32: up to min(G, 32 / G)
//           ways for neighbouring bins, on R / G stores of a lane.
//   fft     chu_fft<M>(img, tw, R, tid): its accesses are k_chu's.
//   filter  lanes run along the image's columns: item (blk, c) stands for the output n = (n0 div M + blk) M + chsy_bin(c), the
//           position whose residue modulo M the passes left in column c, so the outputs of 32 lanes are a permutation inside one
//           contiguous block of M outputs (whole 64-byte segments of it per store) and their image reads are consecutive words
//           of a row.  (Consecutive n would read the columns chu_column(M, n mod M), M / R_1 words apart: 16 dwords at M = 64, an
//           8-way conflict on a ds_read_b64.)  Lanes whose n lie in different frames read different rows of the same column run:
//           word row (M + 1) + c, bank pair (row (M + 1) + c) mod 32, so two lanes meet only where the odd row length carries
//           one onto the other's pair.  Enumerated over the shapes of tests/test_gpu_synthesizer.py: no conflict at I = M
//           (M >= 32) or where a tile is narrower than a half-wave, 2-way in most half-waves otherwise, 3-way in a fifth of
//           them at (32, 7, 33), never more.
//           Every step of the tap loop moves all lanes one row up, so the picture holds for every j.  The tap h[r + j I] is a
//           dword gather from LDS: lanes with the same r read one word (a broadcast), lanes with different r meet only where
//           they differ by a multiple of 64, which needs I > 64.
// Taps sit in LDS, 4 T bytes of the budget: each lane of the filter stage gathers with its own r, and a gather of dwords costs
// LDS one pass where it would cost the vector memory path up to 64 separate words per tap and lane; the price is at most
// 8 frames of F (M = 256, T = 4096).
// LDS: image + table + taps <= CHU_LDS_BUDGET = 64 KiB, two workgroups per CU; F is chsy_frames (channelize_plan.hpp).  The
// J - 1 oldest rows of a workgroup are transformed again by the workgroup before it: (J - 1) / F repeated transforms per
// transform needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channelize_plan.hpp"        // the CHSY_ limits, chsy_frames and chsy_lds_bytes
#include "channelize_uniform_kernels.hpp"

struct ChsyPlace {                   // mfb_synthesizer_placement, as it comes
    int64_t start, src;
    int32_t length, bin;
    float gain;
    int32_t reserved;
};

struct ChsyCall {                    // in device memory, written by mfb_synthesizer_begin
    int32_t nocc;                    // bins with a placement in this call
    int32_t bin[CHU_MAX_BINS];       // their indices, ascending
    int32_t first[CHU_MAX_BINS + 1]; // the placements of bin[o] are first[o] .. first[o + 1] of the sorted list
};

struct ChsyArgs {
    int64_t out_base;
    int64_t q_first;                 // out_base div I
    int32_t out_count;
    int32_t I, T, J, F, R;
};

// the residue s = n mod M that the passes leave in image column c: the inverse of chu_column
// (bin k = q_1 + R_1 (q_2 + ...) stands in column q_1 N / R_1 + the column of q_2 + ... among N / R_1)
template <int N>
__host__ __device__ __forceinline__ int chsy_bin(int c) {
    if constexpr (N == 1) {
        return 0;
    } else {
        constexpr int R = chu_radix(N), L = N / R;
        return c / L + R * chsy_bin<L>(c % L);
    }
}

// Grid: chsy_grid workgroups of CHU_THREADS lanes; dynamic LDS: chsy_lds_bytes(M, I, T, F).  Every index is bounded: the image
// by rho < R and a column < M, the placements by first[o] <= i < first[o + 1] (never empty for o < nocc), the source by
// 0 <= m - start < length with src + length inside it (mfb_synthesizer_begin checks), the taps by t < T, the rows of the filter
// by J - 1 <= row - j <= R - 1 with j <= J - 1, the output by out_base <= n < out_base + out_count.
template <int M>
__global__ __launch_bounds__(CHU_THREADS) void k_chsy(ChsyArgs A, const ChuPlan *__restrict__ P, const ChsyCall *__restrict__ C,
                                                      const ChsyPlace *__restrict__ pl, const float2 *__restrict__ src,
                                                      const float *__restrict__ h, float2 *__restrict__ out) {
    extern __shared__ __align__(16) float2 chsy_lds[];
    const int tid = threadIdx.x, F = A.F, R = A.R, I = A.I, T = A.T;
    chu_cf *img = (chu_cf *)chsy_lds, *tw = img + R * (M + 1);
    float *taps = (float *)(tw + M);
    const int64_t q0 = A.q_first + (int64_t)blockIdx.x * F;
    const int64_t m_lo = q0 - (A.J - 1);
    for (int i = tid; i < R * (M + 1); i += CHU_THREADS) img[i] = (chu_cf){0.0f, 0.0f};
    if (tid < M) tw[tid] = (chu_cf){P->tw[tid].x, P->tw[tid].y};
    for (int t = tid; t < T; t += CHU_THREADS) taps[t] = h[t];
    __syncthreads();
    const int nocc = C->nocc;
    int G = CHU_THREADS;                                     // lanes per occupied bin
    while (G > 1 && G * nocc > CHU_THREADS) G >>= 1;
    const int o = tid / G, sub = tid - o * G;
    if (o < nocc) {
        const int end = C->first[o + 1], col = C->bin[o];
        int i = C->first[o];                                 // the last placement of the bin that starts at or before m_lo, or its first
        for (int hi = end; hi - i > 1;) {
            const int mid = (i + hi) >> 1;
            if (pl[mid].start <= m_lo) i = mid;
            else hi = mid;
        }
        for (; i < end; ++i) {
            const ChsyPlace p = pl[i];
            if (p.start >= m_lo + R) break;
            const int64_t k0 = m_lo - p.start;               // the placement's sample that stands in row 0; -R < k0
            const int64_t left = (int64_t)p.length - k0;     // its end as a row: <= 0 where it ends before m_lo
            const int r0 = k0 < 0 ? (int)-k0 : 0, r1 = left < 0 ? 0 : left < R ? (int)left : R;
            const int64_t at = p.src + k0;                   // row rho holds source[at + rho], r0 <= rho < r1
            for (int rho = r0 + sub; rho < r1; rho += G) {
                float2 v = src[at + rho];
                if (p.gain != 1.0f) {
                    v.x *= p.gain;
                    v.y *= p.gain;
                }
                img[rho * (M + 1) + col] = (chu_cf){v.x, v.y};
            }
        }
    }
    __syncthreads();
    chu_fft<M>(img, tw, R, tid);
    __syncthreads();
    const int64_t n0 = q0 * I, out_end = A.out_base + A.out_count;
    const int64_t n_lo = n0 > A.out_base ? n0 : A.out_base;
    const int64_t n_hi = n0 + (int64_t)F * I < out_end ? n0 + (int64_t)F * I : out_end;
    const int64_t blk0 = n0 / M;                             // (n0 >= 0)
    const int nblk = (int)((n0 + (int64_t)F * I - 1) / M - blk0) + 1;
    for (int item = tid; item < nblk * M; item += CHU_THREADS) {
        const int c = item % M;
        const int64_t n = (blk0 + item / M) * M + chsy_bin<M>(c);
        if (n < n_lo || n >= n_hi) continue;
        const int d = (int)(n - m_lo * I);                   // 0 <= d < R I
        const int row = d / I, r = d - row * I;
        const chu_cf *x = img + row * (M + 1) + c;
        chu_cf acc = (chu_cf){-0.0f, -0.0f};
        for (int t = r; t < T; t += I, x -= M + 1) {
            const float g = taps[t];
            const chu_cf v = *x;
            acc.x = fmaf(g, v.x, acc.x);
            acc.y = fmaf(g, v.y, acc.y);
        }
        out[n - A.out_base] = make_float2(acc.x, acc.y);
    }
}
