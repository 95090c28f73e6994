// Integer IQ samples to complex64 on the device: sc16 (interleaved int16 I, Q -- USRP-class front ends) and sc8 (interleaved
// int8 -- RTL-SDR, HackRF) as they come off the radio, behind the host-to-device copy of a page-locked input buffer or window
// (mfb_set_sample_format).  out[i] = (float(I[i]) * scale, float(Q[i]) * scale) with scale a power of two.
//
// Exact: every int16 / int8 converts to float32 without rounding, and a multiplication by a power of two that stays in the normal
// range changes the exponent only -- so the result is bit for bit numpy's raw.astype(float32) * float32(scale), and whatever the
// compiler makes of the multiply (a stray fused multiply-add with a zero addend included) cannot change it.  Plain C++, no fast
// math.
//
// Memory-bound, no LDS: 4 bytes in and 8 out per sc16 sample, 2 in and 8 out per sc8 sample.  A lane takes one 16-byte group of
// raw samples with one dwordx4 load (4 sc16 or 8 sc8 samples) and writes them with 2 or 4 dwordx4 stores; the grid strides over
// the groups.  The samples behind the last whole group (a window holds nb * stride + overlap samples: any count) go element by
// element, one per lane of the first lanes of the grid.  Both bases are hipMalloc-aligned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int UNPACK_SC16 = 1, UNPACK_SC8 = 2;      // = MFB_SAMPLES_SC16 / _SC8
constexpr int UNPACK_THREADS = 256;
constexpr int UNPACK_MAX_BLOCKS = 2048;

template <int FMT>
struct UnpackFmt;
template <>
struct UnpackFmt<UNPACK_SC16> {
    typedef int16_t part;
    static constexpr int group = 4;                 // samples per 16-byte group
};
template <>
struct UnpackFmt<UNPACK_SC8> {
    typedef int8_t part;
    static constexpr int group = 8;
};

// workgroups for n samples: a lane per group (or per tail sample), capped -- the grid strides over the rest
static inline int unpack_blocks(int fmt, size_t n) {
    const size_t g = fmt == UNPACK_SC16 ? 4 : 8;
    size_t lanes = n / g;
    if (lanes < g) lanes = g;                       // the tail: fewer than `g` samples
    const size_t blocks = (lanes + UNPACK_THREADS - 1) / UNPACK_THREADS;
    return (int)(blocks < (size_t)UNPACK_MAX_BLOCKS ? blocks : (size_t)UNPACK_MAX_BLOCKS);
}

template <int FMT>
__global__ __launch_bounds__(UNPACK_THREADS) void k_unpack(const void *__restrict__ raw, float2 *__restrict__ out, size_t n, float scale) {
    typedef typename UnpackFmt<FMT>::part part;
    constexpr int G = UnpackFmt<FMT>::group;
    const size_t groups = n / G;
    const size_t lane = (size_t)blockIdx.x * UNPACK_THREADS + threadIdx.x, lanes = (size_t)gridDim.x * UNPACK_THREADS;
    const uint4 *in4 = (const uint4 *)raw;
    float4 *out4 = (float4 *)out;
    for (size_t g = lane; g < groups; g += lanes) {
        const uint4 v = in4[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (FMT == UNPACK_SC16) {
            // a word is one sample: I in the low half, Q in the high half
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t a = w[2 * k], b = w[2 * k + 1];
                out4[2 * g + k] = make_float4((float)(int16_t)(a & 0xffffu) * scale, (float)((int32_t)a >> 16) * scale,
                                              (float)(int16_t)(b & 0xffffu) * scale, (float)((int32_t)b >> 16) * scale);
            }
        } else {
            // a word is two samples: I0 Q0 I1 Q1 from the low byte up
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = w[k];
                out4[4 * g + k] = make_float4((float)(int8_t)(a & 0xffu) * scale, (float)(int8_t)((a >> 8) & 0xffu) * scale,
                                              (float)(int8_t)((a >> 16) & 0xffu) * scale, (float)((int32_t)a >> 24) * scale);
            }
        }
    }
    // the samples behind the last whole group, one per lane
    const size_t i = groups * G + lane;
    if (i < n) {
        const part *p = (const part *)raw + 2 * i;
        out[i] = make_float2((float)p[0] * scale, (float)p[1] * scale);
    }
}
