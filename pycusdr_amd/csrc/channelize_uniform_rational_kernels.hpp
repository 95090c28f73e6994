// Rational resampling on the raster (mfb_uniform_channelizer_set_plan_rational): the M bins of channelize_uniform_kernels.hpp,
// bin k centred on k fs / M, each resampled by U / D instead of decimated by D; the selected bins are written.  No reference
// counterpart: the reference takes one narrowband stream per radio process at the rate its bank was built for (pyCuSDR.py:245-251).
//
// Definition: the one of channelize_rational_kernels.hpp with the exact words freq_k = k 2^64 / M (M a power of two).  With real taps
// h[0..T) at the virtual rate U fs, q(m) = (m D) div U and r(m) = (m D) mod U:
//     y_k[m] = sum_{j : r + j U < T} h[r + j U] x[q - j] e^{-2 pi i k (q - j) / M}                  x[n] = 0 for n < 0
//            = sum_{s < M} v_m[s] e^{+2 pi i k s / M}
//     u_m[p] = sum_{i : r + (p + i M) U < T} h[r + (p + i M) U] x[q - p - i M]       p = 0 .. M - 1   (j = p + i M)
//     v_m[s] = u_m[(s + q) mod M]
// because e^{-2 pi i k (q - p - i M) / M} = e^{+2 pi i k ((p - q) mod M) / M}.  This is k_chu's structure with m D replaced by q(m)
// and the taps by the frame's branch g_r[j] = h[r + j U] of ceil((T - r) / U) taps; frames U apart share a branch.  The transform
// (chu_fft<M>), the digit-reversed columns (chu_column), the selection and the output sets are k_chu's.
//
// Pure function of the absolute position.  u_m[p] is the work of one lane, which starts from (-0, -0) and adds its terms in the
// order i = 0, 1, ..., one fused multiply-add per component and tap, exactly the taps with r + (p + i M) U < T and no padded one (a
// branch sum without taps stays (-0, -0)).  r, and the samples read, follow from (U, D, m); the transform's radices, operands and
// order are a function of M alone.  So the order of operations of an output is a function of (M, U, D, T, m): not of F, of the
// frame's slot in the workgroup, of how many frames of a lane share a tap read, of the call's window, of the cut into calls or of
// the selected bins, which only choose what is read back out of the frame's image.  A span computed in one call equals the same
// span computed in any number of calls, from any input window that covers it, with any selection, bit for bit.  With U = 1 every
// operand and every operation is k_chu's: the two kernels give the same bits.
//
// Error bound, first order, per component, with u = 2^-24, Tb = ceil(T / U) and S_m = sum_j |h[r + j U]| |x[q - j]|.  A branch sum
// is a chain of at most ceil(Tb / M) fused multiply-adds per component: its error is at most ceil(Tb / M) u times the branch's own
// sum of |h| |x| in modulus, ceil(Tb / M) u S_m over all branches.  Behind it stands the unchanged transform, whose every value is
// at most S_m in modulus and which rounds by at most 3 u per bit of M (channelize_uniform_kernels.hpp has the count per pass).
//     |device - model| <= (ceil(Tb / M) + 3 log2 M + 2) u S_m
// the 2 for the terms of second order.  Where S_m = 0 every product is a zero, every sum of zeros is a zero: the output is zero
// exactly.  The conversion of sc16 / sc8 is exact.
//
// Shape: a workgroup of 256 lanes makes F consecutive frames m0 .. m0 + F - 1 of all M bins.
//   stage   positions q(m0) - (Tb - 1) .. q(m0 + F - 1) into LDS once, in natural order, converted as chz_load does; zeros below 0
//           and outside the call's input.  (q0, r0) = divmod(m0 D, U) is the one 64-bit division of a workgroup; frame f has
//           r0 + f D = dq_f U + r_f in 32 bits -- r0 + f D < 32 + 128 * 8192 -- and q = q0 + dq_f.  A lane divides once, for its
//           first frame, and from there steps as k_chzr does: a step of its walk adds divmod((256 / M) D, U), the host's, with
//           the carry from r into dq.
//   branch  lane tid owns branch sum p = tid mod M of the frames tid / M + (256 / M) i.  Two frames of that walk share r when
//           (256 / M) (i - i') is a multiple of U, so the lane takes its frames in groups i, i + W, i + 2 W, i + 3 W with
//           W = U / gcd(U, 256 / M): a tap g_r[p + i M] is read once, coalesced along p from the table [r][j] (rows of Tb floats),
//           and serves the four chains (fewer where the walk ends).  Lanes along p read consecutive 8-byte words of the span
//           (descending), as in k_chu.  u goes into the frame's row of the image already shifted, column (p - q) mod M.
//   fft     chu_fft<M>, a barrier between two passes.
//   store   k_chu's: lanes run along m, rows of M + 1 float2.
// LDS: span + image + table <= CHU_LDS_BUDGET; F by chur_frames (channelize_plan.hpp), F M always a multiple of 256.
//
// Bounds.  dq_f <= ((F - 1) D + U - 1) div U, so the staged span has Tb + ((F - 1) D + U - 1) div U positions (chur_span) and tap
// j <= Tb - 1 of frame f reads xs[dq_f + Tb - 1 - j], inside it.  The tap table is read at [r][j] with r + j U < T, j < Tb, inside
// its U Tb floats.  The input is guarded by in_base <= n < in_end, the image by f < F and a column < M, the selection by c < nsel,
// the output by m < out_base + out_count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channelize_uniform_kernels.hpp"

struct ChurArgs {
    int64_t in_base, in_end;         // the call's input holds the positions [in_base, in_end)
    int64_t out_base;
    int32_t out_count;
    int32_t U, D, T, Tb, F, nsel;    // Tb = ceil(T / U): floats per row of the tap table
    int32_t span;                    // staged positions: chur_span(U, D, T, F)
    int32_t share;                   // U / gcd(U, 256 / M): frames that far apart in a lane's walk share a branch
    int32_t share_dq;                // and stand share (256 / M) D / U positions apart, exactly
    int32_t step_dq, step_r;         // divmod((256 / M) D, U): one step of the walk
    int32_t out_stride;              // float2 between two selected bins' outputs
    float scale;
};

// Branch sum p of the NR frames of a lane's walk i0, i0 + istep, ... (frame tid / M + (256 / M) i), which share the branch r: the
// chains of u_m[p], stored shifted.  xs: the staged span, position q(m0) - (Tb - 1) first; g: the table [r][j].
// The first of them is dq0 positions behind q(m0); the next ones follow A.share_dq apart.
template <int M, int NR>
__device__ __forceinline__ void chur_branch(const ChurArgs &A, const float *__restrict__ g, const chu_cf *xs, chu_cf *img, int q0m, int p,
                                            int flane, int i0, int istep, int dq0, int r) {
    constexpr int FSTEP = CHU_THREADS / M;
    chu_cf acc[NR];
    const chu_cf *x[NR];
    int dq[NR];
#pragma unroll
    for (int a = 0; a < NR; ++a) {
        dq[a] = dq0 + a * A.share_dq;
        acc[a] = (chu_cf){-0.0f, -0.0f};
        x[a] = xs + dq[a] + (A.Tb - 1);
    }
    const float *gr = g + r * A.Tb;
    const int nb = (A.T - r + A.U - 1) / A.U;                  // the taps of branch r: j < nb iff r + j U < T
    for (int j = p; j < nb; j += M) {
        const float w = gr[j];
#pragma unroll
        for (int a = 0; a < NR; ++a) {
            const chu_cf v = x[a][-j];
            acc[a].x = fmaf(w, v.x, acc[a].x);
            acc[a].y = fmaf(w, v.y, acc[a].y);
        }
    }
#pragma unroll
    for (int a = 0; a < NR; ++a) {
        const int f = flane + (i0 + a * istep) * FSTEP;
        img[f * (M + 1) + ((p - q0m - dq[a]) & (M - 1))] = acc[a];
    }
}

// Grid: ceil(out_count / F) workgroups of CHU_THREADS lanes; dynamic LDS: chur_lds_bytes(M, U, D, T, F).  The bounds are argued
// above.
template <int M, int FMT>
__global__ __launch_bounds__(CHU_THREADS) void k_chur(ChurArgs A, const ChuPlan *__restrict__ P, const void *__restrict__ raw,
                                                      const float *__restrict__ g, float2 *__restrict__ out) {
    extern __shared__ __align__(16) float2 chur_lds[];
    const int tid = threadIdx.x, F = A.F;
    chu_cf *xs = (chu_cf *)chur_lds, *img = xs + A.span, *tw = img + F * (M + 1);
    const int64_t m0 = A.out_base + (int64_t)blockIdx.x * F;
    const int64_t md = m0 * A.D;
    const int64_t q0 = md / A.U;
    const int r0 = (int)(md - q0 * A.U);
    const int64_t n0 = q0 - (A.Tb - 1);
    for (int p = tid; p < A.span; p += CHU_THREADS) {
        const int64_t n = n0 + p;
        float2 v = make_float2(0.0f, 0.0f);
        if (n >= A.in_base && n < A.in_end) v = chz_load<FMT>(raw, n - A.in_base, A.scale);
        xs[p] = (chu_cf){v.x, v.y};
    }
    if (tid < M) tw[tid] = (chu_cf){P->tw[tid].x, P->tw[tid].y};
    __syncthreads();
    {
        constexpr int FSTEP = CHU_THREADS / M;
        const int p = tid % M, flane = tid / M, nf = F / FSTEP;        // F M is a multiple of 256
        const int q0m = (int)(q0 & (int64_t)(M - 1)), W = A.share;
        // the lane's first frame: r0 + flane D = dqb U + rb, the one 32-bit division of a lane; a step of the walk adds
        // (256 / M) D = step_dq U + step_r with the carry, W steps add share_dq U exactly
        int dqb = (r0 + flane * A.D) / A.U;
        int rb = r0 + flane * A.D - dqb * A.U;
        // the walk i = 0 .. nf - 1 in blocks of 4 W: residue c of a block holds i = base + c + {0, W, 2 W, 3 W}
        for (int base = 0; base < nf; base += 4 * W, dqb += 4 * A.share_dq) {
            int dqc = dqb, rc = rb;
            for (int c = 0; c < W && base + c < nf; ++c) {
                const int i0 = base + c;
                const int n = (nf - 1 - i0) / W + 1;                   // frames of this residue left in the walk
                if (n >= 4) chur_branch<M, 4>(A, g, xs, img, q0m, p, flane, i0, W, dqc, rc);
                else if (n == 3) chur_branch<M, 3>(A, g, xs, img, q0m, p, flane, i0, W, dqc, rc);
                else if (n == 2) chur_branch<M, 2>(A, g, xs, img, q0m, p, flane, i0, W, dqc, rc);
                else chur_branch<M, 1>(A, g, xs, img, q0m, p, flane, i0, W, dqc, rc);
                rc += A.step_r;
                const int carry = rc >= A.U;
                rc -= carry ? A.U : 0;
                dqc += A.step_dq + carry;
            }
        }
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
