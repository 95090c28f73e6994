// Modulator on the device (mfb_modulator_*): bits -> complex64 samples of a LUT modulation, FSK (two rows) or GMSK with a 3-bit
// neighbourhood (eight rows), with one Doppler / frequency-offset increment per frame.  Restates modulator/modulator.py:97-129
// (Modulator.modulate), modulator/modulators/FSK_LUT.py:25-42 and modulator/modulators/GMSK_LUT.py:51-72 of the reference.
//
// The phase is a 64-bit unsigned integer in turns: one sample's increment v rad is quantised once, on the host, in IEEE double
// (t = v / 2pi; t -= floor(t); q = (uint64)(t * 2^64), q = 0 should t have rounded up to 1) and every sum from there on is uint64
// and wraps modulo 2^64.  Wrapping is `mod 2pi` done exactly and integer addition is associative, so every scan order, tile size
// and grid gives the same phase words.  Sample j of symbol s of a frame has
//     phase = init + sum_{u < s} (T[row_u] + spSym * d) + P[row_s][j] + (j + 1) * d
// with P[r][j] = sum_{i <= j} q[r][i] the in-symbol prefix of LUT row r, T[r] = P[r][spSym - 1] its total and d the frame's
// increment.  So the device scans symbols, not samples:
//   k_mod_rows     bits -> row index per symbol (FSK: the bit; GMSK: 4 b[s-1] + 2 b[s] + b[s+1], the bit before a frame's first and
//                  after its last taken as 0 -- never a neighbour frame's bit);
//   k_mod_scan     one workgroup per frame: exclusive scan of T[row] + spSym * d, plus init.  A wave scans with two 32-bit lane
//                  exchanges per value and a 64-bit add (add + add-with-carry) over the sums of four consecutive symbols per lane;
//                  the four wave totals go through LDS; a frame longer than MOD_TILE = 1024 symbols is walked tile by tile with
//                  the running sum carried.  No float anywhere;
//   k_mod_samples  one thread per output sample, one 8-byte store each, neighbouring threads neighbouring samples.  The top three
//                  bits of the phase word pick the octant, the next 32 become the fp32 argument in [0, pi/4] of a sine and a cosine
//                  polynomial -- the whole phase never passes through an fp32 value (a 32-bit turn fraction does not fit 24 mantissa
//                  bits).  The same launch copies the caller's noise array into the pad regions of every frame.
// A batch of frames of different lengths is one launch of each; nothing waits for the host in between.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MOD_THREADS 256              // threads per workgroup of the scan
#define MOD_SPT 4                    // symbols per thread and tile
#define MOD_TILE (MOD_THREADS * MOD_SPT)      // symbols per scan tile
#define MOD_MAX_SPS 1024
#define MOD_MAX_ROWS 8

typedef unsigned long long mod_u64;

// f with off[f] <= i < off[f + 1], off[0] = 0 <= i < off[B] and off strictly increasing
template <class T>
__device__ inline int mod_find_frame(const T *__restrict__ off, int B, T i) {
    int lo = 0, hi = B;          // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mod_rows(const uint8_t *__restrict__ bits, const int32_t *__restrict__ bit_off, int B, int gmsk,
                                                  uint8_t *__restrict__ rows) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= bit_off[B]) return;
    const int b = bits[g] != 0;
    if (!gmsk) {
        rows[g] = (uint8_t)b;
        return;
    }
    const int f = mod_find_frame<int32_t>(bit_off, B, g);
    const int prev = g > bit_off[f] ? bits[g - 1] != 0 : 0;
    const int next = g + 1 < bit_off[f + 1] ? bits[g + 1] != 0 : 0;
    rows[g] = (uint8_t)(4 * prev + 2 * b + next);
}

// inclusive scan over the 64 lanes of a wave, modulo 2^64
__device__ inline mod_u64 mod_wave_scan(mod_u64 v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
        if (lane >= o) v += ((mod_u64)hi << 32) | lo;
    }
    return v;
}

// symbase[g] = init[f] + sum over the frame's symbols before g of (T[row] + sps * d[f]).  Grid: one workgroup per frame; a thread
// owns MOD_SPT consecutive symbols of a tile.
__global__ __launch_bounds__(MOD_THREADS) void k_mod_scan(const uint8_t *__restrict__ rows, const int32_t *__restrict__ bit_off,
                                                          const mod_u64 *__restrict__ T, const mod_u64 *__restrict__ d,
                                                          const mod_u64 *__restrict__ init, int sps, mod_u64 *__restrict__ symbase) {
    __shared__ mod_u64 sT[MOD_MAX_ROWS];
    __shared__ mod_u64 sw[2][MOD_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int b0 = bit_off[f], n = bit_off[f + 1] - b0;
    if (tid < MOD_MAX_ROWS) sT[tid] = T[tid];
    __syncthreads();
    const mod_u64 step = (mod_u64)sps * d[f];
    mod_u64 carry = init[f];
    int buf = 0;
    for (int base = 0; base < n; base += MOD_TILE, buf ^= 1) {
        const int s0 = base + tid * MOD_SPT;
        mod_u64 v[MOD_SPT], mine = 0;
#pragma unroll
        for (int k = 0; k < MOD_SPT; ++k) {
            v[k] = s0 + k < n ? sT[rows[b0 + s0 + k] & (MOD_MAX_ROWS - 1)] + step : 0;
            mine += v[k];
        }
        const mod_u64 inc = mod_wave_scan(mine);
        if ((tid & 63) == 63) sw[buf][wave] = inc;
        __syncthreads();          // sw is double-buffered: one barrier per tile
        mod_u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < MOD_THREADS / 64; ++w) {
            const mod_u64 t = sw[buf][w];
            before += w < wave ? t : 0;
            total += t;
        }
        mod_u64 run = carry + before + inc - mine;
#pragma unroll
        for (int k = 0; k < MOD_SPT; ++k) {
            if (s0 + k < n) symbase[b0 + s0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
}

// sin and cos of x in [0, pi/4], fp32, fused multiply-adds: odd / even minimax polynomials of degree 7 / 8 (the classic single
// precision kernels on this interval; truncation below 2^-27, so the error is the few roundings).  profiles/modulator.md has the
// worst error measured over a dense sweep.
__device__ inline void mod_sincos_oct(float x, float &s, float &c) {
    const float z = x * x;
    const float ps = fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f);
    s = fmaf(x * z, ps, x);
    const float pc = fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f);
    c = fmaf(z * z, pc, fmaf(z, -0.5f, 1.0f));
}

// phase word -> (cos, sin).  Octant o = w >> 61, f = the next 32 bits as a fraction of an octant; odd octants mirror (1 - f, taken
// in integers, so f = 0 gives exactly pi/4).  x = u * pi/4 * 2^-32 with pi/4 split in two floats: one rounding.
__device__ inline float2 mod_phase_to_iq(mod_u64 w) {
    constexpr double K = 0.78539816339744830962 * 0x1p-32;
    constexpr float KH = (float)K;
    constexpr float KL = (float)(K - (double)KH);
    const uint32_t o = (uint32_t)(w >> 61);
    const uint32_t r = (uint32_t)(w >> 29);              // the 32 bits under the octant
    // mirrored: 2^32 - r, which is 2^32 itself for r = 0 -- not a uint32, so that case converts the float constant
    const float u = (o & 1u) ? (r ? (float)(0u - r) : 4294967296.0f) : (float)r;
    const float x = fmaf(u, KH, u * KL);
    float s, c;
    mod_sincos_oct(x, s, c);
    float re, im;
    switch (o) {
        case 0: re = c; im = s; break;
        case 1: re = s; im = c; break;
        case 2: re = -s; im = c; break;
        case 3: re = -c; im = s; break;
        case 4: re = -c; im = -s; break;
        case 5: re = -s; im = -c; break;
        case 6: re = s; im = -c; break;
        default: re = c; im = -s; break;
    }
    return make_float2(re, im);
}

// Frame f occupies out[sample_off[f] .. sample_off[f + 1]): pre = its length - 2 pad - nbits * sps samples noise[0 .. pre) (the
// short-frame pre-pad, modulator.py:121-123), noise[0 .. pad), the signal, noise[0 .. pad) (modulator.py:117-118).  words != nullptr
// (the test seam): the phase word of every signal sample, 0 in the pads.
__global__ __launch_bounds__(256) void k_mod_samples(const uint8_t *__restrict__ rows, const mod_u64 *__restrict__ symbase,
                                                     const int32_t *__restrict__ bit_off, const int64_t *__restrict__ sample_off, int B,
                                                     const mod_u64 *__restrict__ P, const mod_u64 *__restrict__ d, int sps, float rsps,
                                                     int pad, const float2 *__restrict__ noise, float2 *__restrict__ out, mod_u64 *__restrict__ words) {
    // The frames of the workgroup's first and last sample depend on blockIdx alone: uniform bisections.  Nearly always they are
    // the same frame; where a boundary falls inside the workgroup, a thread bisects between the two.
    const int64_t total = sample_off[B];
    const int64_t first = (int64_t)blockIdx.x * 256;
    const int64_t last = first + 255 < total ? first + 255 : total - 1;
    const int64_t i = first + threadIdx.x;
    if (i >= total) return;
    int f = mod_find_frame<int64_t>(sample_off, B, first);
    const int fl = f + mod_find_frame<int64_t>(sample_off + f, B - f, last);
    if (fl != f) f += mod_find_frame<int64_t>(sample_off + f, fl + 1 - f, i);
    const int b0 = bit_off[f];
    const int L = (bit_off[f + 1] - b0) * sps;
    const int len = (int)(sample_off[f + 1] - sample_off[f]);
    const int pre = len - 2 * pad - L;
    const int pos = (int)(i - sample_off[f]);
    float2 v;
    mod_u64 w = 0;
    if (pos < pre) {
        v = noise[pos];
    } else if (pos < pre + pad) {
        v = noise[pos - pre];
    } else if (pos < pre + pad + L) {
        const int k = pos - pre - pad;
        // k / sps through fp32: k < 2^27 and the quotient < 2^17, so the estimate is off by one at the most
        int s = (int)((float)k * rsps);
        int j = k - s * sps;
        if (j < 0) {
            s -= 1;
            j += sps;
        } else if (j >= sps) {
            s += 1;
            j -= sps;
        }
        const int g = b0 + s;
        w = symbase[g] + P[(rows[g] & (MOD_MAX_ROWS - 1)) * sps + j] + (mod_u64)(j + 1) * d[f];
        v = mod_phase_to_iq(w);
    } else {
        v = noise[pos - pre - pad - L];
    }
    out[i] = v;
    if (words) words[i] = w;
}
