// Rational resampling in the channeliser (mfb_channelizer_set_plan_rational): the K channels of channelize_kernels.hpp, resampled
// by U / D instead of decimated by D.  No reference counterpart: the reference takes one narrowband stream per radio process at the
// rate its bank was built for (pyCuSDR.py:245-251).
//
// Definition.  A plan holds an interpolation U and a decimation D (1 <= U <= 32, 2 <= D <= 64, gcd(U, D) = 1, U < D), real taps
// h[0..T) given at the virtual rate U fs (U <= T <= 1024) and K tuning words freq_k, uint64 turns * 2^64 per INPUT sample.  With n
// the absolute input position and m the absolute output position:
//     q(m) = (m D) div U        r(m) = (m D) mod U
//     y_k[m] = sum over j >= 0 with r + jU < T of
//              h[r + jU] x[q - j] e^{-2 pi i phi_k(q - j) / 2^64}      phi_k(n) = n freq_k mod 2^64,  x[n] = 0 for n < 0
// the zero-stuff, filter, keep-every-D-th definition restricted to the products that are not zero.  It is computed as
//     e^{-2 pi i phi_k(q) / 2^64} * sum_j g_k[r + jU] x[q - j]        g_k[t] = h[t] e^{+2 pi i phi_k(t div U) / 2^64}
// which is exact because phi_k is linear in integers; the tables are built once per plan (k_chzr_taps), stored by branch:
// g_k[r + jU] at [k][r][j], rows of Tb = ceil(T / U), so that the taps of one branch are consecutive scalar loads.
//
// The rules of k_chz, word for word: one lane makes one output; the sum starts from (-0, -0); terms are added in the order
// j = 0, 1, ...: for each tap the x.re terms, then the x.im terms; freq_k == 0 uses h itself with one real multiply-add per component
// and is not rotated; a rotation word of 0 multiplies nothing.  A branch runs its own ceil((T - r) / U) taps and no padded ones: a
// padded zero tap would change signed zeros and turn an infinite sample into NaN.  y_k[m] is a pure function of (h, U, D, freq_k,
// the samples it reads, m): neither the order nor the instructions depend on the tile, the class, the window of the call, the
// other channels or the output set.  With U = 1 the definition, the tables, the LDS addresses and the instructions are k_chz's:
// the two kernels give the same bits (tests/test_gpu_channelizer_rational.py holds them to that).
//
// Shape.  Outputs U apart share the branch r and read inputs exactly D apart, so a workgroup of W lanes makes U W consecutive
// outputs m0 .. m0 + U W - 1 in U classes: in class c lane i makes output m0 + c + U i from position q_c + i D with the taps of
// branch r_c, where (q_c, r_c) = divmod((m0 + c) D, U) -- one 64-bit division per workgroup, then r += D, carry into q.  m0 is
// whatever out_base makes it; nothing assumes a multiple of U.  The span all classes read, positions
//     n0 = q_0 - (Tb - 1)  ..  n0 + S - 1,   S = Tb - 1 + W D
// is staged in LDS once, in k_chz's layout [p mod D][p div D] with rows of L float2, L = ceil(S / D) made odd, so every class reads
// consecutive lanes from consecutive words of one row, as k_chz does.
//
// Bounds.  q_c - q_0 <= ((U - 1) D + U - 1) div U <= D - 1 because U < D.  Tap j < ceil((T - r_c) / U) <= Tb of lane i reads the
// image at p = (q_c - q_0) + (Tb - 1) - j + i D: 0 <= p <= (D - 1) + (Tb - 1) + (W - 1) D = S - 1 < D L, row p mod D < D, column
// p div D < L.  The staging loop writes p < S.  A global load is guarded by in_base <= n < in_end, everything else reads as zero
// (mfb_channelizer_begin has checked that what live outputs read is inside or below 0).  A store is guarded by m < out_base +
// out_count <= out_base + out_stride, the channel by the plan's order table (K entries < K).  The tap table is read at
// [k][r_c][j], j < ceil((T - r_c) / U) <= Tb, inside its U Tb entries per channel.
//
// Stores.  The stores of one class are U outputs (8 U bytes) apart and are issued as they are.  The other form -- eight classes of
// a channel group collected in an LDS tile [4][W][8 + 1] and written as runs of eight consecutive outputs, two barriers per tile --
// was built and measured and lost on every plan, by 1.1 to 1.8 times (profiles/channelizer_rational.md): its tile halves W within
// the same LDS budget and it adds the barriers; what the scattered stores cost beside that was not separated.
#pragma once
#include "channelize_kernels.hpp"
#include "channelize_plan.hpp"        // CHZR_MAX_INTERP, and chzr_span / chzr_row_len / chzr_threads for the S and L below

struct ChzrArgs {
    int64_t in_base, in_end;         // the call's input holds the positions [in_base, in_end)
    int64_t out_base;
    int32_t out_count;
    int32_t U, D, T, Tb, L, S;       // Tb = ceil(T / U); L: float2 per LDS row; S: staged positions
    float rD;                        // 1 / D
    int32_t tap_stride, out_stride;  // float2 between two channels' tap tables / outputs
    int32_t ncplx, nreal;
    float scale;
};

// g[k][r][j] = h[t] e^{+2 pi i ((t div U) freq_k) / 2^64} with t = r + j U; (h[t], 0) for a word of 0; (0, 0), never read, for
// t >= T.  Grid: (ceil(U Tb / 256), nchan).
__global__ __launch_bounds__(256) void k_chzr_taps(const float *__restrict__ h, const ChzPlan *__restrict__ P, int U, int T, int Tb,
                                                   int tap_stride, float2 *__restrict__ g) {
    const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (e >= U * Tb) return;
    const int r = e / Tb, j = e - r * Tb, t = r + j * U;
    float2 v = make_float2(0.0f, 0.0f);
    if (t < T) {
        const mod_u64 w = (mod_u64)j * P->freq[k];               // t div U = j
        v = make_float2(h[t], 0.0f);
        if (w != 0) {
            const float2 p = mod_phase_to_iq(w);
            v = make_float2(h[t] * p.x, h[t] * p.y);
        }
    }
    g[(size_t)k * tap_stride + e] = v;
}

// KC channels, P->order[first .. first + KC), for the lane's output m at input position q: the nb taps g of the class's branch
// over the staged span from image position p0 + lane D downwards, the rotation, the store
template <int KC, bool CPLX>
__device__ __forceinline__ void chzr_group(const ChzrArgs &A, const ChzPlan *__restrict__ P, const float2 *__restrict__ taps,
                                           const chz_cf *lane, int first, int nb, int p0, int64_t m, int64_t q, bool live,
                                           float2 *__restrict__ out) {
    chz_cf acc[KC];
    const chz_cf *g[KC];
    int ch[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        ch[i] = P->order[first + i];
        g[i] = (const chz_cf *)taps + (size_t)ch[i] * A.tap_stride;
        acc[i] = (chz_cf){-0.0f, -0.0f};
    }
    int r = p0 % A.D, c = p0 / A.D;                    // tap j reads row (p0 - j) mod D, column (p0 - j) div D + lane
    // CHZ_UNROLL taps at a time, as chz_group: the order of the additions is j = 0 .. nb - 1 in either loop
    int t = 0;
    for (; t + CHZ_UNROLL <= nb; t += CHZ_UNROLL) {
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
    for (; t < nb; ++t) {
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
            const mod_u64 w = (mod_u64)0 - (mod_u64)q * P->freq[ch[i]];                // -phi_k(q)
            if (w != 0) {
                const float2 p = mod_phase_to_iq(w);
                y = make_float2(fmaf(-acc[i].y, p.y, acc[i].x * p.x), fmaf(acc[i].y, p.x, acc[i].x * p.y));
            }
        }
        out[(size_t)ch[i] * A.out_stride + (m - A.out_base)] = y;
    }
}

template <bool CPLX>
__device__ __forceinline__ void chzr_groups(const ChzrArgs &A, const ChzPlan *__restrict__ P, const float2 *__restrict__ taps,
                                            const chz_cf *lane, int first, int n, int nb, int p0, int64_t m, int64_t q, bool live,
                                            float2 *__restrict__ out) {
    for (; n >= 4; n -= 4, first += 4) chzr_group<4, CPLX>(A, P, taps, lane, first, nb, p0, m, q, live, out);
    if (n & 2) {
        chzr_group<2, CPLX>(A, P, taps, lane, first, nb, p0, m, q, live, out);
        first += 2;
    }
    if (n & 1) chzr_group<1, CPLX>(A, P, taps, lane, first, nb, p0, m, q, live, out);
}

// Grid: ceil(out_count / (U W)) workgroups of W = blockDim.x lanes; dynamic LDS: D * L float2.  The bounds are argued above.
template <int FMT>
__global__ __launch_bounds__(CHZ_MAX_THREADS) void k_chzr(ChzrArgs A, const ChzPlan *__restrict__ P, const void *__restrict__ raw,
                                                          const float2 *__restrict__ taps, float2 *__restrict__ out) {
    extern __shared__ __align__(16) float2 chzr_lds[];
    const int tid = threadIdx.x, W = blockDim.x;
    const int64_t m0 = A.out_base + (int64_t)blockIdx.x * W * A.U;
    const int64_t end = A.out_base + A.out_count;
    const int64_t md = m0 * A.D;
    const int64_t q0 = md / A.U;
    const int64_t n0 = q0 - (A.Tb - 1);
    for (int p = tid; p < A.S; p += W) {
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
        chzr_lds[r * A.L + q] = v;
    }
    __syncthreads();
    const chz_cf *lane = (const chz_cf *)chzr_lds + tid;
    int rc = (int)(md - q0 * A.U);                     // the class's branch, and its first lane's position as an offset from q0
    int dq = 0;
    for (int c = 0; c < A.U; ++c) {
        if (m0 + c >= end) break;                      // no lane of this class, or of a later one, is live
        const int64_t m = m0 + c + (int64_t)A.U * tid;
        const int64_t q = q0 + dq + (int64_t)tid * A.D;
        const bool live = m < end;
        const int nb = (A.T - rc + A.U - 1) / A.U;
        const float2 *g = taps + rc * A.Tb;
        chzr_groups<true>(A, P, g, lane, 0, A.ncplx, nb, dq + A.Tb - 1, m, q, live, out);
        chzr_groups<false>(A, P, g, lane, A.ncplx, A.nreal, nb, dq + A.Tb - 1, m, q, live, out);
        rc += A.D;
        const int adv = rc / A.U;
        dq += adv;
        rc -= adv * A.U;
    }
}
