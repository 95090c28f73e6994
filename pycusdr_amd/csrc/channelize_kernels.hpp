// Channeliser on the device (mfb_channelizer_*): one wideband capture -> K channels, each tuned to baseband, low-pass filtered with
// the plan's real taps and decimated by D.  No reference counterpart: the reference takes one narrowband stream per radio process
// (pyCuSDR.py:245-251) and leaves tuning and decimation to whoever feeds it.
//
// Definition, n the absolute position in the wideband stream, m in a channel's output stream, freq_k uint64 turns * 2^64 per
// input sample (the convention of mod_kernels.hpp; a negative frequency is the two's complement):
//     phi_k(n) = n * freq_k                                                     (uint64, wrapping modulo 2^64)
//     y_k[m]   = sum_{t < T} h[t] x[m D - t] e^{-2 pi i phi_k(m D - t) / 2^64}       x[n] = 0 for n < 0
// phi_k is linear in integers, so phi_k(m D - t) = phi_k(m D) - phi_k(t) exactly, and the kernel computes
//     y_k[m]   = e^{-2 pi i phi_k(m D) / 2^64} * sum_{t < T} g_k[t] x[m D - t]       g_k[t] = h[t] e^{+2 pi i phi_k(t) / 2^64}
// with the table g_k built once per plan (k_chz_taps) and one phasor per output, both through mod_phase_to_iq.
//
// Pure function of the absolute position: an output is the work of one lane, which starts from (-0, -0) -- the one start that
// leaves the first product's bits alone, signed zeros included -- and adds the T products in the order t = 0 .. T - 1, two fused
// multiply-adds per component and tap (first the x.re terms, then the x.im terms), then rotates.  Neither the order nor the
// instructions depend on the tile the output falls in, on the window of the call or on the other channels of the plan: a span
// computed in one call equals the same span computed in any number of calls, bit for bit.
// Exact cases (selects): freq_k == 0 takes h itself as taps, one real multiply-add per component and tap, and is not rotated; a
// rotation word of 0 multiplies nothing.  So h = [1], freq = 0 gives y[m] = x[m D] bit for bit.
//
// Shape: a workgroup of W = 64, 128 or 256 lanes produces W consecutive outputs of every channel.  It stages the span it reads,
// positions m0 D - (T - 1) .. (m0 + W - 1) D, in LDS once, converting sc16 / sc8 on the way (float(int) * scale, as k_unpack) and
// writing zeros for positions outside the call's input (below 0, or behind its end for the outputs of a last tile that are not
// stored); the channels then reuse it, four at a time: per tap one LDS read of x feeds the accumulators of four channels.
// LDS layout: by polyphase branch, position p of the span at [p mod D][p div D], rows of L float2 (L odd).  For tap t every lane
// reads row (T - 1 - t) mod D at column (T - 1 - t) div D + lane: consecutive lanes, consecutive 8-byte words, so a ds_read_b64
// of a 32-lane half touches each of the 64 banks once -- no conflict (the natural layout [p] has a lane stride of 8 D bytes: bank
// (2 D lane) mod 64, a 16-way conflict at D = 16).  The staging writes of 16 consecutive lanes go to up to 16 rows, 2 L dwords
// apart: L odd makes 2 L r mod 32 distinct for r < 16, every one of the 32 write banks once.
// The taps are uniform: g_k[t] is read with scalar loads and enters the packed fp32 multiply-adds as their scalar operand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channelize_plan.hpp"        // the limits, and how wide a workgroup is (chz_threads, chz_row_len)
#include "mod_kernels.hpp"

#define CHZ_UNROLL 8                 // taps per trip of the inner loop
#define CHZ_FMT_CF32 0              // = MFB_SAMPLES_CF32 / _SC16 / _SC8
#define CHZ_FMT_SC16 1
#define CHZ_FMT_SC8 2

typedef float chz_cf __attribute__((ext_vector_type(2)));

struct ChzPlan {                     // in device memory, written by mfb_channelizer_set_plan
    mod_u64 freq[CHZ_MAX_CHANNELS];
    int32_t order[CHZ_MAX_CHANNELS]; // the channels with freq != 0 first (ncplx of them), then those with freq == 0
};

struct ChzArgs {
    int64_t in_base, in_end;         // the call's input holds the positions [in_base, in_end)
    int64_t out_base;
    int32_t out_count;
    int32_t D, T, L;                 // L: float2 per LDS row
    float rD;                        // 1 / D
    int32_t tap_stride, out_stride;  // float2 between two channels' tap tables / outputs
    int32_t ncplx, nreal;
    float scale;
};

// g[k][t] = h[t] e^{+2 pi i (t freq_k) / 2^64}; (h[t], 0) for a word of 0.  Grid: (ceil(T / 256), nchan).
__global__ __launch_bounds__(256) void k_chz_taps(const float *__restrict__ h, const ChzPlan *__restrict__ P, int T, int tap_stride,
                                                  float2 *__restrict__ g) {
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (t >= T) return;
    const mod_u64 w = (mod_u64)t * P->freq[k];
    float2 v = make_float2(h[t], 0.0f);
    if (w != 0) {
        const float2 p = mod_phase_to_iq(w);
        v = make_float2(h[t] * p.x, h[t] * p.y);
    }
    g[(size_t)k * tap_stride + t] = v;
}

// acc += x.re * g: (acc.re + x.re g.re, acc.im + x.re g.im); g uniform, in scalar registers
__device__ __forceinline__ void chz_fma_re(chz_cf &acc, chz_cf x, chz_cf g) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(x), "s"(g));
}
// acc += i x.im * g: (acc.re - x.im g.im, acc.im + x.im g.re)
__device__ __forceinline__ void chz_fma_im(chz_cf &acc, chz_cf x, chz_cf g) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "+v"(acc) : "v"(x), "s"(g));
}
// acc += x * g.re (real taps): (acc.re + x.re g.re, acc.im + x.im g.re)
__device__ __forceinline__ void chz_fma_real(chz_cf &acc, chz_cf x, chz_cf g) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(x), "s"(g));
}

template <int FMT>
__device__ __forceinline__ float2 chz_load(const void *__restrict__ raw, int64_t i, float scale) {
    if (FMT == CHZ_FMT_CF32) return ((const float2 *)raw)[i];
    if (FMT == CHZ_FMT_SC16) {
        const uint32_t a = ((const uint32_t *)raw)[i];           // I in the low half, Q in the high half
        return make_float2((float)(int16_t)(a & 0xffffu) * scale, (float)((int32_t)a >> 16) * scale);
    }
    const uint32_t a = ((const uint16_t *)raw)[i];
    return make_float2((float)(int8_t)(a & 0xffu) * scale, (float)(int8_t)(a >> 8) * scale);
}

// tap t of KC channels: the x.re terms of every channel, then the x.im terms (four independent chains between the two halves of one)
template <int KC, bool CPLX>
__device__ __forceinline__ void chz_tap(chz_cf (&acc)[KC], chz_cf x, const chz_cf *(&g)[KC], int t) {
    if (CPLX) {
#pragma unroll
        for (int i = 0; i < KC; ++i) chz_fma_re(acc[i], x, g[i][t]);
#pragma unroll
        for (int i = 0; i < KC; ++i) chz_fma_im(acc[i], x, g[i][t]);
    } else {
#pragma unroll
        for (int i = 0; i < KC; ++i) chz_fma_real(acc[i], x, g[i][t]);
    }
}

// KC channels, P->order[first .. first + KC), for the lane's output m: the sums over the staged span, the rotation, the store
template <int KC, bool CPLX>
__device__ __forceinline__ void chz_group(const ChzArgs &A, const ChzPlan *__restrict__ P, const float2 *__restrict__ taps,
                                          const chz_cf *lane, int first, int64_t m, bool live, float2 *__restrict__ out) {
    chz_cf acc[KC];
    const chz_cf *g[KC];
    int ch[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        ch[i] = P->order[first + i];
        g[i] = (const chz_cf *)taps + (size_t)ch[i] * A.tap_stride;
        acc[i] = (chz_cf){-0.0f, -0.0f};
    }
    int r = (A.T - 1) % A.D, c = (A.T - 1) / A.D;      // tap t reads row (T - 1 - t) mod D, column (T - 1 - t) div D + lane
    // CHZ_UNROLL taps at a time: their LDS reads and the scalar loads of their taps are issued together, one wait for all.  The
    // order of the additions is t = 0 .. T - 1 in either loop.
    int t = 0;
    for (; t + CHZ_UNROLL <= A.T; t += CHZ_UNROLL) {
        chz_cf x[CHZ_UNROLL];
#pragma unroll
        for (int u = 0; u < CHZ_UNROLL; ++u) {
            x[u] = lane[r * A.L + c];
            const bool wrap = r == 0;
            r = wrap ? A.D - 1 : r - 1;
            c -= wrap;
        }
#pragma unroll
        for (int u = 0; u < CHZ_UNROLL; ++u) chz_tap<KC, CPLX>(acc, x[u], g, t + u);
    }
    for (; t < A.T; ++t) {
        const chz_cf x = lane[r * A.L + c];
        chz_tap<KC, CPLX>(acc, x, g, t);
        const bool wrap = r == 0;
        r = wrap ? A.D - 1 : r - 1;
        c -= wrap;
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        float2 y = make_float2(acc[i].x, acc[i].y);
        if (CPLX) {
            const mod_u64 w = (mod_u64)0 - (mod_u64)(m * A.D) * P->freq[ch[i]];       // -phi_k(m D)
            if (w != 0) {
                const float2 p = mod_phase_to_iq(w);
                y = make_float2(fmaf(-acc[i].y, p.y, acc[i].x * p.x), fmaf(acc[i].y, p.x, acc[i].x * p.y));
            }
        }
        out[(size_t)ch[i] * A.out_stride + (m - A.out_base)] = y;
    }
}

template <bool CPLX>
__device__ __forceinline__ void chz_groups(const ChzArgs &A, const ChzPlan *__restrict__ P, const float2 *__restrict__ taps,
                                           const chz_cf *lane, int first, int n, int64_t m, bool live, float2 *__restrict__ out) {
    for (; n >= 4; n -= 4, first += 4) chz_group<4, CPLX>(A, P, taps, lane, first, m, live, out);
    if (n & 2) {
        chz_group<2, CPLX>(A, P, taps, lane, first, m, live, out);
        first += 2;
    }
    if (n & 1) chz_group<1, CPLX>(A, P, taps, lane, first, m, live, out);
}

// Grid: ceil(out_count / W) workgroups of W = blockDim.x lanes; dynamic LDS: D * L float2.  Every global index is bounded: the
// input by in_base <= n < in_end, the output by m < out_base + out_count, the LDS image by p < (W - 1) D + T <= D L.
template <int FMT>
__global__ __launch_bounds__(CHZ_MAX_THREADS) void k_chz(ChzArgs A, const ChzPlan *__restrict__ P, const void *__restrict__ raw,
                                                         const float2 *__restrict__ taps, float2 *__restrict__ out) {
    extern __shared__ __align__(16) float2 chz_lds[];
    const int tid = threadIdx.x, W = blockDim.x;
    const int64_t m0 = A.out_base + (int64_t)blockIdx.x * W;
    const int64_t n0 = m0 * A.D - (A.T - 1);
    const int span = (W - 1) * A.D + A.T;
    for (int p = tid; p < span; p += W) {
        const int64_t n = n0 + p;
        float2 v = make_float2(0.0f, 0.0f);
        if (n >= A.in_base && n < A.in_end) v = chz_load<FMT>(raw, n - A.in_base, A.scale);
        // p / D through fp32: p < 2^15, so the estimate is off by one at the most
        int q = (int)((float)p * A.rD);
        int r = p - q * A.D;
        if (r < 0) {
            q -= 1;
            r += A.D;
        } else if (r >= A.D) {
            q += 1;
            r -= A.D;
        }
        chz_lds[r * A.L + q] = v;
    }
    __syncthreads();
    const int64_t m = m0 + tid;
    const bool live = m < A.out_base + A.out_count;
    const chz_cf *lane = (const chz_cf *)chz_lds + tid;
    chz_groups<true>(A, P, taps, lane, 0, A.ncplx, m, live, out);
    chz_groups<false>(A, P, taps, lane, A.ncplx, A.nreal, m, live, out);
}
