// wrap_kernels.hpp -- the 256-point filter-side search (segf_body, SUMQ = 2) with the wrap-around energy on the matrix cores.
//
// segf_body scores a (bin, segment) as  L sum_k |A[k]|^2 Q_b[k] - sum_f sum_{n in [V, L)} |v_{b,f}[n]|^2 : a Parseval total shared by the
// bin's filters, minus the energy of the L - V outputs whose filter support wraps around the segment, which it gets from a product and a
// pruned inverse transform per (bin, filter) on the vector ALUs.  Those outputs are short dot products over the segment's edges:
//     v_{b,f}[V + n'] = N sum_{r < T} h_{b,f}[r] x_seg[(n' - r) mod L],   n' < L - V,   h_{b,f}[r] = tap_f[r] e^{+2 pi i s_b r / N}
// (the Te - 1 = L - V rotation of segment_spectra_shifted: output V + n' reads samples n' - r, i.e. the last T - 1 and the first L - V of
// the segment).  For one segment that is the matrix product  Toeplitz(x_seg)[L - V x T] . H_b[T x MU], in real form
//     [Xr Xi] [[Hr, Hi], [-Hi, Hr]]   (K = 2T real rows, 2 MU <= 16 columns: one 16-column tile per bin, columns (filter, re / im)),
// run here as v_mfma_f32_16x16x32_f16: row tile rt (16 outputs) x K-step kk (taps 16 kk ... 16 kk + 15, real and imaginary halves of the
// window).  The Toeplitz block of (rt, kk) depends on rt - kk only, so a segment has RT + KT - 1 distinct A fragments.
// The instantiated shape (PV = 13 valid register slots, KT = 3) serves banks of 34 ... 48 taps: with 33 taps a segment has 14 valid
// slots, 49 taps need a fourth K-step (search_plan.hpp, wrap_kt).  Taps 16 KT - 1 down to T are zero rows of the B fragments, and the
// window is zeroed below offset -(T - 1), so that the segment's scale comes from the samples the product reads.
//
// fp16 precision from a split: each operand is scaled by a power of two chosen from the data (the segment window: its largest
// |component|; the bin's taps: theirs, host side) into [2^14, 2^15), and split into hi = fp16(v) and lo = fp16(v - hi).  Three products
// lo.hi + hi.lo + hi.hi accumulate in fp32 (lo.lo, ~2^-22 relative, is dropped).  Because both scales are powers of two taken from the
// data, scaling the input by 2^k leaves the fp16 operands and the accumulators bit for bit the same and the score scales exactly.
//
// Everything else is segf_body's: the XCD-aware groups of the grid, the unmixed forward transform (via the inverse one on swapped
// samples), the Parseval total from pp = |A|^2 and Q, and the PRESUM store (row 0 carries the (bin, slot) sum, the other rows are not written).
// A bin's number depends on its own tables and the slot's samples only, summed in one fixed order: the same bits whichever bins share
// the rectangle, whatever the grid or the batch.
//
// The rectangle of bins x slots is this form's own (search_plan.hpp, fsm_plan): a slot's prologue -- samples, window, forward transform and
// the 160 fragment registers -- runs with the matrix pipe idle and nothing else on the SIMD, so a wave takes its group's whole share
// of bins, up to 32 a chunk, and pays the prologue once for them (profiles/r12_wrap_slots.md: C2 1.13x over 16 bins) -- up to 64 a
// chunk where the launch is long enough to keep four rounds of waves (profiles/r14_wrap_wide.md: the fixed part of a slot is 9.4 k
// cycles beside 2.13 k a bin).  The groups of that plan are groups of bins, four of them up to 256 bins: the four waves of a workgroup
// then walk the same bins on four slots and share the table fetches in the CU's vector cache, which four chunks of one slot do not.  The loads
// of a slot are not carried into the next: 32 registers of samples across the bin loop cost more than their latency (r12).
//
// The window in LDS (profiles/segw_fixed_costs.md).  A segment's window is 96 samples x 2 components, and a wave's 160 fragment
// registers read each of them 13 times over.  So the split is made once: when the segment's scale is known (the 16-lane maximum), each
// lane scales and splits its own 12 components -- ldexp, hi = fp16(v), lo = fp16(v - hi), the operations and the order the fragments
// always had -- and stores each as one word {hi, lo} into planes [segment][re | im][window index], the bytes the complex window took.
// A fragment is then eight consecutive words of the lane's plane (ds_read2_b32: word alignment only; the 32 lanes of an access touch 24
// consecutive words, no bank twice) and one v_perm_b32 per register: the low halves of two neighbours for hi, the high halves for lo.
//
// Where the values live and how a step of the bin loop issues (profiles/r13_wrap_issue.md).  With one wave on the SIMD a 16x16x32 MFMA
// holds the vector issue for 8 of its 16 cycles and every other instruction costs about 4, so a gap between two MFMAs hides two
// instructions and pays for every further one.  The library is compiled with -mllvm -amdgpu-mfma-vgpr-form (k_segw is its only kernel
// with an MFMA): the products accumulate in arch VGPRs, where the vector ALUs of `finish` read them with no copy, and what only the
// MFMA reads -- the 160 fragment registers and both sets of B fragments -- is pinned to the accumulation registers by empty asm
// statements with an "a" constraint (the fragments are written there once, as they are built; the B tables are loaded there).  A
// step's 108 gaps are then filled by sched_group_barrier: scalar address arithmetic and the row of the bin before (carried as a
// value and stored ahead of the table fetches, so that no wait at the head of a step covers a store just issued) in the first four,
// the ten table fetches of the bin after next one to a gap, and the squares, the reduction, the lane sums and the Parseval total of
// the bins at hand one or two to a gap through all the others.  The row store is a buffer store with the lanes >= 1 out of range,
// in place of a branch; packed fp32 instructions, which cost a gap more than the two they replace, are kept apart by "v" constraints.
// No operation on a score changed: the same operands in the same order.
#pragma once
#include "seg_kernels.hpp"

typedef _Float16 seg_h8 __attribute__((ext_vector_type(8)));
typedef float seg_f4 __attribute__((ext_vector_type(4)));

struct SegWArgs {
    SegFArgs f;          // the segf_body arguments (presum form: Qs set, rows counting equally)
    const u32x4 *Wb;     // [Dtot][KT][2 = hi, lo][64 lanes]: B fragments, 8 fp16 per lane (filter_taps.hpp, wrap_taps_shifted)
    const int *Wexp;     // [Dtot]: 2 log2(N) - 2 e_b, the bin's power of two of the wrap energy (e_b: its taps' scale)
    int T;               // taps of the layout (T <= 16 KT)
};

template <int PV, int KT>
struct SegWCfg {
    static constexpr int L = 256, PPL = 16, NT = 16, CT = 4;
    static constexpr int RT = PPL - PV;               // row tiles = wrap outputs / 16
    static constexpr int ND = RT + KT - 1;            // distinct Toeplitz blocks of a segment
    static constexpr int OFF = 16 * KT - 1;           // window index of sample offset 0: t = n' - r in [-(16 KT - 1), 16 RT - 1]
    static constexpr int WSTR = 16 * (RT + KT);       // window elements per segment (one spare)
    static_assert(RT >= 1 && RT + KT <= PPL, "the window is the first RT and the last KT register slots of a lane");
    // one wave per SIMD: the four segments' fragments (160 registers) and two sets of B fragments stay in the accumulation registers,
    // two sets of accumulators (96) in the arch VGPRs; two waves spill.  The matrix loop is 27 k cycles per slot, the forward transform ~1 k.
    static constexpr int WAVES = 1;
    static constexpr size_t lds_bytes() {
        return (size_t)SegCfg<256>::LDS_ELEMS * sizeof(cf) + (size_t)(SegCfg<256>::BLOCK / 64) * CT * WSTR * sizeof(cf);
    }
};

// a bin's tables in registers: the B fragments (hi, lo) and its Parseval weights
template <int KT>
struct SegWBin {
    seg_h8 hi[KT], lo[KT];
    cf q[8];
};

template <int PV, int KT>
DEVI void segw_body(const SegWArgs &w, const int blk) {
    static_assert(MFB_FFT_FUSED, "the fused 256-point transform");
    using Cfg = SegCfg<256>;
    using WC = SegWCfg<PV, KT>;
    constexpr int L = 256, NT = Cfg::NT, CT = Cfg::CT, PPL = Cfg::PPL, RT = WC::RT, ND = WC::ND, OFF = WC::OFF, WSTR = WC::WSTR;
    static_assert(NT == WC::NT && CT == WC::CT && PPL == WC::PPL, "256-point geometry");
    const SegFArgs &a = w.f;
    extern __shared__ __attribute__((aligned(16))) cf lds[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int g = lane % NT;
    const int col = lane / NT;
    cf *mylds = lds + wave * Cfg::LDS_PER_TEAM + col * padlen(L);
    // this wave's segment windows, split: [segment][re | im][window index] words {hi, lo} (the bytes of CT * WSTR complex samples)
    unsigned *wpl = reinterpret_cast<unsigned *>(lds + Cfg::LDS_ELEMS + wave * CT * WSTR);
    F256Regs f256;
    f256_setup(f256, a.twL + L, g);

    // ---- this wave's rectangle (segf_body) ----
    const int grp = blk % a.nsg;
    const int u = (blk / a.nsg) * (Cfg::BLOCK / 64) + wave;
    const int per_sc = a.nblk * a.nbc;
    const int sc = u / per_sc, rest = u - sc * per_sc;
    const int bk = rest / a.nbc, bc = rest - bk * a.nbc;
    const int gs0 = a.gbins ? 0 : (int)((long long)grp * a.nslots / a.nsg);
    const int glen = a.gbins ? a.nslots : (int)((long long)(grp + 1) * a.nslots / a.nsg) - gs0;
    const int gb0 = a.gbins ? (int)((long long)grp * a.dper / a.nsg) : 0;
    const int gblen = a.gbins ? (int)((long long)(grp + 1) * a.dper / a.nsg) - gb0 : a.dper;
    const int s0 = __builtin_amdgcn_readfirstlane(a.slot0 + gs0 + sc * a.fs);
    const int s1 = __builtin_amdgcn_readfirstlane(min(a.slot0 + gs0 + glen, s0 + a.fs));
    const int jb0 = __builtin_amdgcn_readfirstlane(gb0 + bc * a.fb);
    const int jb1 = __builtin_amdgcn_readfirstlane(min(gb0 + gblen, jb0 + a.fb));
    if (sc >= a.nsc || s0 >= s1 || jb0 >= jb1 || bk >= a.nblk) return;           // (wave-uniform)

    const unsigned nmask = (unsigned)a.N - 1u;
    const auto xr = mk_rsrc(a.x + (size_t)bk * (size_t)a.xstride, (unsigned)a.N * sizeof(cf));
    const auto qr = mk_rsrc(a.Qs, (unsigned)a.dper * (unsigned)(L * sizeof(float)));
    const auto br = mk_rsrc(w.Wb, (unsigned)a.dper * (unsigned)(KT * 2 * 64 * 16));
    auto load_q = [&](cf (&dst)[PPL / 2], int so) {
#pragma unroll
        for (int jj = 0; jj < PPL / 4; ++jj)
            buf_load_cf2(qr, g * 4 * (int)sizeof(float) + jj * NT * 4 * (int)sizeof(float), so, dst[2 * jj], dst[2 * jj + 1]);
    };
    auto load_b = [&](seg_h8 (&hi)[KT], seg_h8 (&lo)[KT], int so) {
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            hi[kk] = __builtin_bit_cast(seg_h8, __builtin_amdgcn_raw_buffer_load_b128(br, lane * 16 + kk * 2 * 1024, so, 0));
            lo[kk] = __builtin_bit_cast(seg_h8, __builtin_amdgcn_raw_buffer_load_b128(br, lane * 16 + (kk * 2 + 1) * 1024, so, 0));
        }
    };
    constexpr int so_x = NT * (int)sizeof(cf);
    const int T = w.T;
    // fragment coordinates of this lane: A[row i16][k = 8 q + j], k < 16 the real halves of the window, k >= 16 the imaginary ones
    const int i16 = lane & 15, q = lane >> 4;
    const bool im_half = q >= 2;
    const int qo = 8 * (q & 1);
    // ... and the lowest word of its plane that it reads: element 7 of Toeplitz block 0 (window index i16 - qo + 8 with OFF = 16 KT - 1)
    static_assert(OFF - 16 * (KT - 1) - 7 - 8 >= 0 && 16 * (ND - 1) + 7 + 15 + OFF - 16 * (KT - 1) - 7 < WSTR, "the fragments stay inside a plane");
    const unsigned *wfrag = wpl + (im_half ? WSTR : 0) + (i16 - qo + OFF - 16 * (KT - 1) - 7);

    // the bins' powers of two of the wrap energy, lane j holding bin jb0 + j's: fetched once (the samples' loads wait for it), so that
    // no bin waits for a load at the head of its products
    const bool one_chunk = jb1 - jb0 <= 64;
    int wexl = jb0 + lane < jb1 ? w.Wexp[jb0 + lane] : 0;
    // the row store (PRESUM: lane 0 the sum into row 0; rows >= 1 are not written, k_finalize counts them as zeros without reading
    // them) as a buffer store: bytes from bin to bin, and each lane's offset -- lanes >= 1 beyond any buffer size, so that the
    // hardware drops them
    const int pstep = __builtin_amdgcn_readfirstlane(a.MU * a.parts * (int)sizeof(float));
    const int pvo = lane == 0 ? 0 : 0x7FFFFFFF;

    for (int slot = s0; slot < s1; ++slot) {
        cf v[PPL];
        {
            const unsigned e0 = (unsigned)(slot * CT + col) * (unsigned)a.V + (unsigned)g;
            const unsigned last = (unsigned)(slot * CT + CT - 1) * (unsigned)a.V + (unsigned)L;      // wave-uniform
            if (__builtin_amdgcn_readfirstlane(last <= (unsigned)a.N ? 1 : 0)) {
                const int vo_x = (int)(e0 * sizeof(cf));
#pragma unroll
                for (int i = 0; i < PPL; ++i) {
                    const cf t = buf_load_cf(xr, vo_x, i * so_x);
                    v[i] = mkc(t.y, t.x);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PPL; ++i) {
                    const cf t = buf_load_cf(xr, (int)(((e0 + (unsigned)(NT * i)) & nmask) * sizeof(cf)), 0);
                    v[i] = mkc(t.y, t.x);
                }
            }
        }
        // ---- the segment's wrap window -> LDS: sample offsets t in [-(T - 1), L - V) (register slots < RT and >= PPL - KT), zero below
        // Every sample of the window is scaled and split ONCE, by the lane that holds it, as soon as the segment's scale is known: the
        // word {hi, lo} goes into the plane [segment][re | im][window index], and the fragments below are reads of those words.
        int ea;
        {
            cf ws[RT + KT];
            float mx = 0.f;
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                ws[i] = mkc(v[i].y, v[i].x);
                mx = fmaxf(mx, fmaxf(fabsf(ws[i].x), fabsf(ws[i].y)));
            }
#pragma unroll
            for (int i = PPL - KT; i < PPL; ++i) {
                const int t = g + NT * i - L;
                const cf s = t >= -(T - 1) ? mkc(v[i].y, v[i].x) : mkc(0.f, 0.f);
                ws[RT + i - (PPL - KT)] = s;
                mx = fmaxf(mx, fmaxf(fabsf(s.x), fabsf(s.y)));
            }
            // the segment's largest |component| (its 16 lanes): max is exact in any order
#pragma unroll
            for (int m = 1; m < NT; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
            int e;
            (void)frexpf(mx, &e);             // mx = f 2^e, f in [0.5, 1): mx 2^(15 - e) in [2^14, 2^15)  (mx = 0: e = 0)
            ea = 15 - e;
            auto split = [&](float comp) {
                const float sv = __builtin_ldexpf(comp, ea);
                const _Float16 h = (_Float16)sv;
                const _Float16 l = (_Float16)(sv - (float)h);
                return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
            };
            unsigned *myw = wpl + col * 2 * WSTR;
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                myw[g + NT * i + OFF] = split(ws[i].x);
                myw[WSTR + g + NT * i + OFF] = split(ws[i].y);
            }
#pragma unroll
            for (int i = PPL - KT; i < PPL; ++i) {
                const int t = g + NT * i - L;
                if (t + OFF >= 0) {
                    myw[t + OFF] = split(ws[RT + i - (PPL - KT)].x);
                    myw[WSTR + t + OFF] = split(ws[RT + i - (PPL - KT)].y);
                }
            }
        }
        xsync<1>();
        cf A[PPL];
        {
            auto keep = [&](int, cf val, auto, auto nu) { A[decltype(nu)::value / NT] = val; };
            fft256_fused<0, PPL>(v, mylds, g, f256, keep);
        }
        cf pp[PPL / 2];
#pragma unroll
        for (int j = 0; j < PPL / 2; ++j) {
            const cf p0 = A[2 * j] * A[2 * j], p1 = A[2 * j + 1] * A[2 * j + 1];
            pp[j] = mkc(p0.x + p0.y, p1.x + p1.y);
        }
        // ---- the A fragments of the CT segments: ND Toeplitz blocks each, from the split window.  Element j of block di is window
        // index 16 (di - (KT - 1)) + i16 - qo + OFF - j: eight consecutive words of the lane's plane, a register of the hi fragment the
        // low halves of two neighbours, a register of the lo fragment their high halves ----
        seg_h8 ahi[CT][ND], alo[CT][ND];
        int eseg[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            eseg[c] = __builtin_amdgcn_readlane(ea, NT * c);
            const unsigned *wc = wfrag + c * 2 * WSTR;
#pragma unroll
            for (int di = 0; di < ND; ++di) {
                u32x4 fh, fl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned e0 = wc[16 * di + 7 - 2 * r], e1 = wc[16 * di + 6 - 2 * r];      // elements j = 2 r, 2 r + 1
                    fh[r] = __builtin_amdgcn_perm(e1, e0, 0x05040100u);
                    fl[r] = __builtin_amdgcn_perm(e1, e0, 0x07060302u);
                }
                ahi[c][di] = __builtin_bit_cast(seg_h8, fh);
                alo[c][di] = __builtin_bit_cast(seg_h8, fl);
                asm("" : "+a"(ahi[c][di]));
                asm("" : "+a"(alo[c][di]));
            }
        }
        xsync<1>();       // the windows are rewritten by the next slot

        // ---- the bins: bin jb + 1's products issue with bin jb's squares, reduction and store between them (two sets of accumulators
        // and of bin tables, taking turns), so that the matrix pipe does not idle while the vector ALUs finish a bin.  A bin's arithmetic
        // is what it was: the same operations on the same operands in the same order.
        for (int jc = jb0; jc < jb1; jc += 64) {
            if (!one_chunk) {       // a rectangle of more than 64 bins: fetched per chunk, and waited for here, not at the head of a bin
                wexl = jc + lane < jb1 ? w.Wexp[jc + lane] : 0;
                __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0)
            }
            const int jc1 = min(jb1, jc + 64);
            const auto pr = mk_rsrc(a.partials + ((size_t)(a.part_row0 + bk * a.dper + jc) * a.MU) * a.parts + slot, 64u * (unsigned)pstep);
            SegWBin<KT> b0, b1;
            seg_f4 acc0[CT][RT], acc1[CT][RT];
            // carried from step to step: the row of the bin before, stored ahead of the next step's table fetches (nothing yet: every lane
            // out of range)
            unsigned pend = 0u;
            int pendvo = 0x7FFFFFFF;
            // the Parseval total of the bin's filters (segf_body)
            auto parseval = [&](const SegWBin<KT> &b) {
                float tx[2] = {0.f, 0.f}, ty[2] = {0.f, 0.f};
#pragma unroll
                for (int j = 0; j < PPL / 2; ++j) {
                    tx[j & 1] = __builtin_fmaf(pp[j].x, b.q[j].x, tx[j & 1]);
                    ty[j & 1] = __builtin_fmaf(pp[j].y, b.q[j].y, ty[j & 1]);
                    asm("" : "+v"(tx[j & 1]), "+v"(ty[j & 1]));
                }
                float s0 = tx[0] + ty[0];
                asm("" : "+v"(s0));
                return s0 + (tx[1] + ty[1]);
            };
            auto fetch = [&](SegWBin<KT> &b, int bin) {
                load_b(b.hi, b.lo, bin * (KT * 2 * 1024));
                load_q(b.q, bin * (L * (int)sizeof(float)));
            };
            // the wrap products: per segment, RT row tiles x KT K-steps x (lo.hi, hi.lo, hi.hi)
            auto products = [&](seg_f4 (&acc)[CT][RT], SegWBin<KT> &b) {
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) asm("" : "+a"(b.hi[kk]), "+a"(b.lo[kk]));
#pragma unroll
                for (int c = 0; c < CT; ++c) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        seg_f4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk) {
                            const int di = rt - kk + KT - 1;
                            t = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo[c][di], b.hi[kk], t, 0, 0, 0);
                            t = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[c][di], b.lo[kk], t, 0, 0, 0);
                            t = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[c][di], b.hi[kk], t, 0, 0, 0);
                        }
                        acc[c][rt] = t;
                    }
                }
            };
            // the wrap energy, squared and summed in a fixed order, off the Parseval total; then the wave's 64 values in segf_body's
            // fixed order: quads, the four quads of a row, the four rows
            auto finish = [&](const seg_f4 (&acc)[CT][RT], float tot, int jb) {
                const int wexp = __builtin_amdgcn_readlane(wexl, jb - jc);
                float wacc = 0.f;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    float sq[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const seg_f4 t = acc[c][rt];
                        sq[rt] = __builtin_fmaf(t.x, t.x, t.y * t.y) + __builtin_fmaf(t.z, t.z, t.w * t.w);
                        asm("" : "+v"(sq[rt]));
                    }
                    float s = sq[0];
#pragma unroll
                    for (int rt = 1; rt < RT; ++rt) s += sq[rt];
                    wacc += __builtin_ldexpf(s, wexp - 2 * eseg[c]);
                }
                float sv = __builtin_fmaf((float)L, tot, -wacc);
                sv += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sv), 0xB1, 0xF, 0xF, true));       // quad_perm [1,0,3,2]
                sv += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sv), 0x4E, 0xF, 0xF, true));       // quad_perm [2,3,0,1]
                sv += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sv), 0x124, 0xF, 0xF, true));      // row_ror:4
                sv += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sv), 0x128, 0xF, 0xF, true));      // row_ror:8
                const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), 0));
                const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), 16));
                const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), 32));
                const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), 48));
                float r01 = r0 + r1;
                asm("" : "+v"(r01));
                return r01 + (r2 + r3);
            };
            auto row = [&](float total) { return lane == 0 ? __float_as_uint(total * a.scale) : 0u; };
            auto store = [&](unsigned val, int vo, int so) { __builtin_amdgcn_raw_buffer_store_b32(val, pr, vo, so, 0); };
            auto row_off = [&](int jb) { return __builtin_amdgcn_readfirstlane(max(jb - jc, 0)) * pstep; };      // (jb = jc - 1: nothing carried yet)
            // one bin's products with the bin before's finish between them, at most two other instructions to a product (16 cycles of the
            // matrix pipe, of which the MFMA holds the issue for 8); the row carried from the step before is stored and the tables of
            // the bin after (clamped to the chunk: the last one is fetched twice, into the set nobody reads) are requested first, all
            // memory instructions of a step within its first 14 gaps
            auto step = [&](seg_f4 (&accn)[CT][RT], SegWBin<KT> &bn, const seg_f4 (&accp)[CT][RT], SegWBin<KT> &bp, float totp, int jb) {
                store(pend, pendvo, row_off(jb - 1));
                fetch(bp, min(jb + 2, jc1 - 1));
                products(accn, bn);
                const float total = finish(accp, totp, jb);
                const float totn = parseval(bn);
                pend = row(total);
                pendvo = pvo;
#pragma unroll
                for (int i = 0; i < CT * RT * KT * 3; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);        // one MFMA
                    if (i < 4) {
                        if (i == 2) {
                            __builtin_amdgcn_sched_group_barrier(0x40, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x4, 1, 0);
                        } else {
                            __builtin_amdgcn_sched_group_barrier(0x4, 2, 0);
                        }
                    } else if (i < 14) {
                        __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x6, 1, 0);
                    } else if ((i & 3) && i < 96) {
                        __builtin_amdgcn_sched_group_barrier(0x6, 1, 0);
                    } else {
                        __builtin_amdgcn_sched_group_barrier(0x6, 2, 0);
                    }
                }
                return totn;
            };
            fetch(b0, jc);
            fetch(b1, min(jc + 1, jc1 - 1));
            float tot0 = parseval(b0), tot1 = 0.f;
            products(acc0, b0);
            int jb = jc;
            while (true) {
                if (jb + 1 >= jc1) {
                    store(pend, pendvo, row_off(jb - 1));
                    store(row(finish(acc0, tot0, jb)), pvo, row_off(jb));
                    break;
                }
                tot1 = step(acc1, b1, acc0, b0, tot0, jb);
                ++jb;
                if (jb + 1 >= jc1) {
                    store(pend, pendvo, row_off(jb - 1));
                    store(row(finish(acc1, tot1, jb)), pvo, row_off(jb));
                    break;
                }
                tot0 = step(acc0, b0, acc1, b1, tot1, jb);
                ++jb;
            }
        }
    }
}
template <int PV, int KT>
__global__ void __launch_bounds__(SegCfg<256>::BLOCK) __attribute__((amdgpu_waves_per_eu(SegWCfg<PV, KT>::WAVES, SegWCfg<PV, KT>::WAVES)))
k_segw(SegWArgs w) {
    segw_body<PV, KT>(w, (int)blockIdx.x);
}
