// Soft combiner on the device (mfb_combiner_*): align several receivers' bit streams against a master's new bits and vote
// bit by bit.  Restates the deterministic core of softCombiner.py:665-798 (correlate), :570-618 (_doVoteN), :623-662 (_doVote2).
//
// The alignment correlation is exact.  The streams are 0/1, so lag k of
//     x[k] = sum_{j < min(Lc, n)} bT[(j + k) mod N] * bM[j]
// is a count: with the master packed LSB-first into 32-bit words M[w] and the slave, zero-padded to N bits, into S[.]
//     x[32 q + r] = sum_w popc( M[w] & alignbit(S[w + q + 1], S[w + q], r) )
// (alignbit = the 32-bit window r bits into the pair).  No fp32, no twiddles, no tolerance: the same reasoning as
// sync_kernels.hpp.  The slave is stored once, NW = max(N / 32, 1) words, and addressed with the mask NW - 1, which is the
// circular wrap of the reference's FFT form; a slave of N < 32 bits is packed periodically so that the one word wraps alike.
//
// Work split of k_cmb_xcorr: a thread owns one q and keeps the 32 sums of r = 0..31 in registers; a workgroup owns 256
// consecutive q (blockIdx.x) and every gridDim.y-th tile of 64 master words (blockIdx.y).  Per tile the 256 + 64 + 1 slave
// words and the 64 master words are staged in LDS: thread t reads word t + w, neighbouring threads neighbouring words
// (conflict-free ds_read_b32), the master word is uniform (a broadcast).  The partial sums of the tiles of one workgroup are
// transposed through LDS (row stride 33) and added to x with coalesced int32 atomics; integer addition commutes, so every
// split over words and workgroups gives the same bits.  x is zeroed before the launch.
//
// Master words past min(Lc, n) are skipped and the last one is masked; Lc comes from device memory (the result record's
// out_len while a call runs), because an earlier slave may have shortened the master.  Nothing here waits for the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CMB_TOPK 15          // values the decision looks at (softCombiner.py:709)
#define CMB_QB 256           // q per workgroup = threads
#define CMB_TILE 64          // master words per tile
#define CMB_SEG 4096         // lags per workgroup of the first top-15 stage (16 per thread)
#define CMB_RUNNING (-1)     // mfb_combine_result.status while a call is in flight
#define CMB_LUT_STRIDE 8192  // per voter count: 4096 bits | 4096 trust bytes

typedef unsigned long long cmb_key;      // (value << 32) | ~index: the largest key is the largest value at the lowest index

// uint8 0/1 -> one bit per element, LSB first: bit i of the packed stream is src[i & wrapmask] (0 beyond n).  One ballot per
// 64 elements; lane 0 of the wave stores its two words.
__global__ __launch_bounds__(256) void k_cmb_pack(const uint8_t *__restrict__ src, int n, uint32_t wrapmask, uint32_t *__restrict__ dst,
                                                  int nwords) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t s = i & wrapmask;
    const bool bit = (i >> 5) < (uint32_t)nwords && s < (uint32_t)n && src[s] != 0;
    const unsigned long long b = __ballot(bit);
    if ((threadIdx.x & 63u) == 0u) {
        const uint32_t w = i >> 5;
        if (w < (uint32_t)nwords) dst[w] = (uint32_t)b;
        if (w + 1 < (uint32_t)nwords) dst[w + 1] = (uint32_t)(b >> 32);
    }
}

__global__ void k_cmb_init(mfb_combine_result *res, int Lm, int nslaves) {
    int32_t *p = (int32_t *)res;
    for (unsigned i = threadIdx.x; i < sizeof(mfb_combine_result) / sizeof(int32_t); i += blockDim.x) p[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        res->status = CMB_RUNNING;
        res->out_len = Lm;              // the current master length Lc while the call runs
        res->num_slaves = nslaves;
    }
}

// x[k] += this workgroup's share; see the head of the file.  res == nullptr: the test seam, L = Lfix.
__global__ __launch_bounds__(256) void k_cmb_xcorr(const uint32_t *__restrict__ M, const uint32_t *__restrict__ S, uint32_t nwmask, int n,
                                                   int nlags, const mfb_combine_result *res, int Lfix, int32_t *__restrict__ x) {
    __shared__ uint32_t sS[CMB_QB + CMB_TILE + 1];
    __shared__ uint32_t sM[CMB_TILE];
    __shared__ int32_t sT[CMB_QB * 33];
    int L = Lfix;
    if (res) {
        if (res->status != CMB_RUNNING) return;
        L = res->out_len;
    }
    if (n < L) L = n;
    const int MW = (L + 31) >> 5;
    if ((int)blockIdx.y * CMB_TILE >= MW) return;
    const int tid = threadIdx.x;
    const uint32_t q0 = blockIdx.x * (uint32_t)CMB_QB;
    int32_t acc[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[r] = 0;
    for (int t0 = blockIdx.y * CMB_TILE; t0 < MW; t0 += gridDim.y * CMB_TILE) {
        __syncthreads();
        for (int i = tid; i < CMB_QB + CMB_TILE + 1; i += 256) sS[i] = S[(q0 + (uint32_t)t0 + (uint32_t)i) & nwmask];
        if (tid < CMB_TILE) {
            const int w = t0 + tid;
            uint32_t m = 0;
            if (w < MW) {
                m = M[w];
                const int rem = L - 32 * w;
                if (rem < 32) m &= (1u << rem) - 1u;
            }
            sM[tid] = m;
        }
        __syncthreads();
        uint32_t lo = sS[tid];
        const int wend = MW - t0 < CMB_TILE ? MW - t0 : CMB_TILE;
#pragma unroll 2
        for (int w = 0; w < wend; ++w) {
            const uint32_t hi = sS[tid + w + 1];
            const uint32_t m = sM[w];
#pragma unroll
            for (int r = 0; r < 32; ++r) acc[r] += __builtin_popcount(m & __builtin_amdgcn_alignbit(hi, lo, r));
            lo = hi;
        }
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) sT[tid * 33 + r] = acc[r];
    __syncthreads();
    for (int i = 0; i < 32; ++i) {
        const int e = tid + 256 * i;
        const int v = sT[(e >> 5) * 33 + (e & 31)];
        const long long lag = (long long)q0 * 32 + e;
        if (lag < (long long)nlags && v != 0) atomicAdd(&x[lag], v);
    }
}

__device__ inline cmb_key cmb_wave_max(cmb_key v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const cmb_key u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// The CMB_TOPK largest keys of up to 16 per thread x 256 threads, in descending order, into top[] (shared): repeated arg-max
// with removal, as the reference's loop (softCombiner.py:713-716).  Keys are unique (they carry the index) except the padding
// key 0, which only ever stands for the value 0.  Per round: a maximum per wave by lane exchange, the four of them through
// sred[2][4] -- two buffers taken in turn, so that one barrier per round suffices.
__device__ inline void cmb_block_top(cmb_key (&k)[16], cmb_key *sred, cmb_key *top) {
    const int tid = threadIdx.x;
    for (int round = 0; round < CMB_TOPK; ++round) {
        cmb_key best = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) best = k[j] > best ? k[j] : best;
        best = cmb_wave_max(best);
        cmb_key *s = sred + (round & 1) * 4;
        if ((tid & 63) == 0) s[tid >> 6] = best;
        __syncthreads();
        cmb_key win = s[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) win = s[w] > win ? s[w] : win;
        if (tid == 0) top[round] = win;
        if (win != 0) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (k[j] == win) k[j] = 0;
        }
    }
    __syncthreads();
}

// Stage 1: every workgroup's candidates of its CMB_SEG lags.
__global__ __launch_bounds__(256) void k_cmb_top_seg(const int32_t *__restrict__ x, int nlags, const mfb_combine_result *res,
                                                     cmb_key *__restrict__ cand) {
    __shared__ cmb_key sred[8];
    __shared__ cmb_key top[CMB_TOPK];
    if (res && res->status != CMB_RUNNING) return;
    cmb_key k[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t idx = blockIdx.x * (uint32_t)CMB_SEG + (uint32_t)j * 256u + threadIdx.x;
        k[j] = idx < (uint32_t)nlags ? (((cmb_key)(uint32_t)x[idx]) << 32) | (cmb_key)(0xFFFFFFFFu - idx) : 0;
    }
    cmb_block_top(k, sred, top);
    if (threadIdx.x < CMB_TOPK) cand[blockIdx.x * CMB_TOPK + threadIdx.x] = top[threadIdx.x];
}

// numpy's float64 sum of 13 values (pairwise routine, n < 128: eight partial sums, then the rest in order).  Contraction is switched
// off by pragma in the two functions that make cond: HIP's __dadd_rn / __dmul_rn are plain `x + y` / `x * y` in the headers, and
// under the compiler's default -ffp-contract=fast-honor-pragmas they fuse with their neighbours after inlining (t * t + u * u and
// mean + vm * sd became v_fma_f64, one rounding fewer than numpy: cond differed in the last bit).  The operators below carry no
// contract flag, so neither a product made here nor one handed in can be fused into these sums.
__device__ inline double cmb_sum13(const double *a) {
#pragma clang fp contract(off)
    double r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (int i = 8; i < 13; ++i) r = r + a[i];
    return r;
}

// cond = mean(val[2:]) + vm * std(val[2:]) as numpy computes it in float64 (softCombiner.py:720): every line one correctly rounded
// operation (the division and the square root expand to IEEE-exact sequences of their own), none fused with the next
__device__ inline double cmb_cond(const double *v, double vm) {
#pragma clang fp contract(off)
    const double mean = cmb_sum13(v + 2) / 13.0;
    double d[13];
    for (int i = 0; i < 13; ++i) {
        const double t = v[i + 2] - mean;
        d[i] = t * t;
    }
    const double sd = __dsqrt_rn(cmb_sum13(d) / 13.0);
    const double scaled = vm * sd;
    return mean + scaled;
}

// Stage 2 and the decision: one workgroup merges ncand <= 4096 candidates; thread 0 computes
//     cond = mean(val[2:]) + vm * std(val[2:])          (float64, softCombiner.py:720)
// writes slave `slave`'s record and updates Lc (res->out_len), the status and the matched list.
__global__ __launch_bounds__(256) void k_cmb_decide(const cmb_key *__restrict__ cand, int ncand, mfb_combine_result *res, int slave, int n,
                                                    double vm, int min_length) {
    __shared__ cmb_key sred[8];
    __shared__ cmb_key top[CMB_TOPK];
    if (res->status != CMB_RUNNING) return;
    cmb_key k[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = j * 256 + (int)threadIdx.x;
        k[j] = i < ncand ? cand[i] : 0;
    }
    cmb_block_top(k, sred, top);
    if (threadIdx.x != 0) return;
    mfb_combine_slave *r = &res->slave[slave];
    double v[CMB_TOPK];
    for (int i = 0; i < CMB_TOPK; ++i) {
        r->val[i] = (int32_t)(top[i] >> 32);
        v[i] = (double)r->val[i];
    }
    const int idx0 = (int)(0xFFFFFFFFu - (uint32_t)top[0]);
    const double cond = cmb_cond(v, vm);
    int Lc = res->out_len;
    r->evaluated = 1;
    r->cond = cond;
    r->idx0 = idx0;
    r->matched = v[0] > cond ? 1 : 0;
    r->avail = 0;
    if (r->matched) {
        int avail = n - idx0 < Lc ? n - idx0 : Lc;
        if (avail < 0) avail = 0;
        r->avail = avail;
        if (avail < min_length) {
            res->status = MFB_COMBINE_NOTHING;
        } else {
            if (avail < Lc) Lc = avail;
            res->matched_slaves[res->matched_count] = slave;
            res->matched_count += 1;
            res->out_len = Lc;
        }
    }
    r->lc_after = Lc;
}

struct CmbVoteArgs {
    const uint8_t *bits[MFB_COMBINE_MAX_SLAVES];
    const int8_t *trust[MFB_COMBINE_MAX_SLAVES];
    int n[MFB_COMBINE_MAX_SLAVES];
};

__device__ inline uint32_t cmb_code(uint8_t bit, int8_t t) {
    return (bit ? 4u : 0u) + (t < -1 ? 0u : t == -1 ? 1u : t == 0 ? 2u : 3u);
}

// One launch after the last slave.  An output bit's column state -- per voter the bit and the trust class {< -1, -1, 0, > 0},
// three bits each, the master lowest -- indexes the tables the host built from the numpy form of _doVoteN / _doVote2.
__global__ __launch_bounds__(256) void k_cmb_vote(const mfb_combine_result *res, const uint8_t *__restrict__ mb, const int8_t *__restrict__ mt,
                                                  CmbVoteArgs a, const uint8_t *__restrict__ lut, uint8_t *__restrict__ ob,
                                                  int8_t *__restrict__ ot) {
    __shared__ uint8_t sb[4096];
    __shared__ int8_t st[4096];
    if (res->status != CMB_RUNNING) return;
    const int K = res->matched_count, Lc = res->out_len;
    if (K > 0) {
        const int entries = 1 << (3 * (K + 1));
        const uint8_t *t = lut + (size_t)(K - 1) * CMB_LUT_STRIDE;
        for (int i = threadIdx.x; i < entries; i += 256) {
            sb[i] = t[i];
            st[i] = (int8_t)t[4096 + i];
        }
    }
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Lc) return;
    if (K == 0) {
        ob[j] = mb[j];
        ot[j] = mt[j];
        return;
    }
    uint32_t s = cmb_code(mb[j], mt[j]);
    for (int v = 0; v < K; ++v) {
        const int sl = res->matched_slaves[v];
        const int p = res->slave[sl].idx0 + j;
        const uint32_t c = p < a.n[sl] ? cmb_code(a.bits[sl][p], a.trust[sl][p]) : 0u;
        s |= c << (3 * (v + 1));
    }
    ob[j] = sb[s];
    ot[j] = st[s];
}

__global__ void k_cmb_finish(mfb_combine_result *res) {
    if (res->status == CMB_RUNNING) {
        res->status = res->matched_count > 0 ? MFB_COMBINE_COMBINED : MFB_COMBINE_MASTER_ONLY;
    } else {
        res->out_len = 0;
        res->matched_count = 0;
    }
}
