// search_plan.hpp -- everything that DECIDES how the segment search runs, and nothing that launches: host arithmetic on a dozen
// integers, no HIP call, no handle.  resolve_segments settles path, segment length and basis for a bank; plan_search takes every launch
// and table decision of one search, once.  bank_search_api.hpp fills a SearchInputs from a handle (search_inputs) and consumes the plan: the
// launches, mfb_get_search_info and the eager table build read the SAME answer, and mfb_debug_search_plan shows it to the tests.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include "../../include/mfbank.h"
#include "seg_kernels.hpp"
#include "wrap_kernels.hpp"

typedef mfb_plan_inputs SearchInputs;   // what the decisions depend on, and nothing else (include/mfbank.h)
typedef mfb_seg_plan SegPlan;           // geometry of one k_seg launch
typedef mfb_search_plan SearchPlan;
enum { SEARCH_NONE = 0, SEARCH_SEG = 1, SEARCH_SEGF256 = 2, SEARCH_SEGF2048 = 3, SEARCH_SEGW = 4 };    // SearchPlan::form

// The A/B switches of the environment, read here and nowhere else, once per process: inputs with the switch fields set, the rest 0.
//   MFB_SEG_FSM=0         keeps the search on seg_body (profiles/r06_fft_ops.md)
//   MFB_SEG_WRAP_MFMA=0   keeps the 256-point search's wrap-around energy on the vector ALUs (segf_body), off the matrix cores (k_segw)
//   MFB_SEG_FSM_RECT="fb,fs"  sets the rectangle a wave takes (bins x slots);  MFB_SEG_FSM_GROUP=0|1  groups of slots | of bins
inline const SearchInputs &search_env() {
    static const SearchInputs env = [] {
        SearchInputs e = {};
        e.fsm = e.wrap_mfma = 1, e.group = -1;
        if (const char *s = getenv("MFB_SEG_FSM")) e.fsm = atoi(s) != 0;
        if (const char *s = getenv("MFB_SEG_WRAP_MFMA")) e.wrap_mfma = atoi(s) != 0;
        if (const char *s = getenv("MFB_SEG_FSM_RECT")) sscanf(s, "%d,%d", &e.rect_fb, &e.rect_fs);
        if (const char *s = getenv("MFB_SEG_FSM_GROUP")) e.group = atoi(s);
        return e;
    }();
    return env;
}

// ---- path, segment length, basis -------------------------------------------------------------------
// Valid outputs per complete segment: the largest multiple of NT = L / (points per lane) not above L - T + 1, so that
// they are whole register slots (seg_kernels.hpp); 0 if fewer than half of a segment would be valid.
#define SEG_LOG2L_MAX 13      // 8192-point segments: filters of up to 4097 taps
#define SEG_TWOPASS_COST 6.45  // the two-pass path in the units of seg_cost (ms per block at C2's geometry)
inline int seg_valid(int l, int T) {
    const int L = 1 << l, ppl = seg_ppl(L), NT = L / ppl;
    const int pv = (L - T + 1) / NT;
    return pv >= ppl / 2 ? pv * NT : 0;
}
// Relative cost of one segment point per filter, MEASURED on MI355X at C2 (time x V / L, 48 taps, D = 256,
// M = 8; tools/seg_probe.py): the 256-point kernel is by far the cheapest per point (one twiddled pass,
// three waves per SIMD, phase table in LDS), so it wins whenever at least ~2/3 of a segment is valid; the
// cost of a valid output is this divided by the segment efficiency V / L.  Re-measured late in round 3 at the settled
// clock and with a quiet host (profiles/r03_ramp.md: the first ~30 ms after an idle spell run 8-20 % slow, and a probe whose
// own BLAS threads get the process throttled starves the device the same way -- some earlier tables carried both effects):
// GMSK bank, 256 ... 4096 points: 1.597 / 2.128 / 2.070 / 2.443 / 2.648 ms; CC11xx bank (384 taps) on five devices:
// 2048 points 2.69-2.77 ms, 4096 points 2.90-2.96 ms (the 2048-point kernel gained 5 % from one team per workgroup);
// BPSK bank (80 taps), 256 / 512 / 1024 points: 3.74 / 4.28 / 4.15 ms.  Figures with 32 workgroups per CU in the grid.
// Round 4: the 2048-point kernel became one wave per segment with one LDS exchange per transform (seg_kernels.hpp, W32):
// 2.51 against 2.72 ms on one device for the 384-tap bank (profiles/r04_long_filter.md), hence 2.20 -> 2.03.  8192 points (one
// eight-wave team per CU, four passes): 4.67 ms at 2049 taps, 5.05 at 2050, 5.48 at 3000, 6.61 at 4097 -> 3.45 per point; in
// these units the two-pass path costs 6.45 whatever the filter (6.5 ms), so the longest filters of the range stay there.
inline double seg_cost(int l, int T, int MU = 8) {
    // Round 6 (fused transforms, the shift on the filters' side for 256 and 2048 points; gpurun_out/r06_taps.txt: random banks at C2,
    // lengths forced beside the chosen one): 256 points 1.49 ms at 64 taps, 1.74 at 96 -> 1.10; 2048 points 1.90 at 100 taps, 2.28 at 512,
    // 2.68 at 768, 3.24 at 1025 -> 1.75 (1.62 ... 1.78: dead register slots are pruned as the valid share shrinks); 4096 points 2.98 at
    // 768 taps, 3.53 at 1150 -> 2.43.  The 2048-point kernel now keeps 650 ... ~850 taps that went to 4096 points (2.68 against 2.98 ms
    // at 768 taps); the hand-over from 256 points stays just under 100 taps (1.91 against 1.90 ms at 100).
    // ... and once more with the complement second pass (gpurun_out/r06_taps2.txt), whose cost falls with the share of valid slots:
    // 256 points 1.28 ms at 48 taps, 1.44 at 64, 1.60 at 80, 1.75 at 88 / 96 (10 valid slots: no complement) -> 1.08; 2048 points 1.45 ms
    // at 64 taps, 1.60 at 72 ... 100, 2.45 at 640, 2.69 at 768, 3.16 at 900 -> 1.60.  The hand-over from 256 to 2048 points moves from
    // just under 100 taps to 81 (1.75 against 1.60 ms at 88 and 96 taps; a tie at 64 ... 80), 2048 points keep everything up to 1025.
    static const double per_point[14] = {0, 0, 0, 0, 0, 0, 0, 0, MFB_FFT_FUSED ? (MFB_SEG_COMPLEMENT ? 1.08 : 1.10) : 1.35, 1.94, 2.02,
                                         MFB_SEG_W32 ? (MFB_FFT_FUSED ? (MFB_SEG_COMPLEMENT ? 1.60 : 1.75) : 2.03) : 2.20,
                                         MFB_FFT_FUSED ? 2.43 : 2.55, 3.45};
    const int V = seg_valid(l, T);
    if (!V) return 1e30;
    // (the 2048-point kernel takes the filter-side shift and the complement pass for up to 8 filters per bin only: with more it runs
    // round 6's fused transforms on seg_body -- 2.32 ms on the 384-tap bank, 1.89 per point)
    const double pp = (l == 11 && MFB_SEG_W32 && MFB_FFT_FUSED && MU > 8) ? 1.89 : per_point[l];
    return pp * (double)(1 << l) / (double)V;
}

inline int choose_segl(const SearchInputs &in, bool may_decline) {
    int best = 0;
    double bc = 1e30;
    for (int l = 8; l <= SEG_LOG2L_MAX; ++l) {
        if (!seg_valid(l, in.T) || (4 << l) > in.N) continue;    // at least half of every segment valid, >= 4 segments
        const double cost = seg_cost(l, in.T, in.MU);
        if (cost < bc) {
            bc = cost;
            best = l;
        }
    }
    // barely half of an 8192-point segment valid: the two-pass path is no slower (unless the caller insists on segments)
    if (may_decline && bc > SEG_TWOPASS_COST) return 0;
    return best;
}

// path and segment length from the request and the analysed bank.  ok = false: segments were demanded and this bank (or block) has
// none (MFB_ERR_UNSUPPORTED).  T: taps the segments are laid out for (>= the bank's); basis: with the span rank in.MB.
struct Segments {
    int path, segl, V, T, Q, basis;
    bool ok;
};
inline Segments resolve_segments(const SearchInputs &in) {
    int l = 0;
    if (in.path_req != MFB_PATH_TWOPASS && in.segl_req) {
        if (in.segl_req >= 8 && in.segl_req <= SEG_LOG2L_MAX && seg_valid(in.segl_req, in.T) && (2 << in.segl_req) <= in.N) l = in.segl_req;
    } else if (in.path_req != MFB_PATH_TWOPASS) {
        l = choose_segl(in, in.path_req == MFB_PATH_AUTO);
    }
    if (!l) return Segments{MFB_PATH_TWOPASS, 0, 0, 0, 0, MFB_BASIS_FILTERS, in.path_req != MFB_PATH_SEGMENT};
    const int V = seg_valid(l, in.T);
    // opt-in span basis of the SUM_ALL search (filter_taps.hpp): rank(C) filters instead of M
    const bool span = in.basis_req == MFB_BASIS_SPAN && in.sum_all && in.MB > 0;
    return Segments{MFB_PATH_SEGMENT, l, V, (1 << l) - V + 1, (in.N + V - 1) / V, span ? MFB_BASIS_SPAN : MFB_BASIS_FILTERS, true};
}

// ---- k_seg's launches ------------------------------------------------------------------------------
// Decomposition of one launch over `nslots` slots (a slot = CT neighbouring segments, one team
// iteration): nsg segment groups (8 = one per XCD under round-robin placement), each with wpg workgroups
// = bsplit Doppler streams x ssplit slot sub-ranges (x TPW teams).
struct SegGeom {
    int NT, TEAM, CT, TPW, WPT;
    bool wave_sync;
};
inline SegGeom seg_geom(int segl) {
    const int L = 1 << segl, NT = L / seg_ppl(L), TEAM = NT < 64 ? 64 : NT;
    return SegGeom{NT, TEAM, TEAM / NT, seg_block_threads(NT) / TEAM, TEAM / 64, NT <= 64};
}
// Dynamic LDS of k_seg<1 << segl, mode, .> at mpb filters per pass: the one statement its attribute and its launches take.
constexpr int seg_mpb_cap(int segl) { return segl == 13 ? 8 : SEG_MPB_MAX; }   // (8192 points: 157 KiB with 8 filters per pass is all a CU has)
inline int seg_lds_bytes(int segl, int mode, int mpb) {
    const int m = mode == SEG_REDUCE ? mpb : 0;
    const size_t by_segl[] = {SegCfg<256>::lds_bytes(m),  SegCfg<512>::lds_bytes(m),  SegCfg<1024>::lds_bytes(m),
                              SegCfg<2048>::lds_bytes(m), SegCfg<4096>::lds_bytes(m), SegCfg<8192>::lds_bytes(m)};
    return (int)by_segl[segl - 8];
}
// (SegPlan::igroups > 1: the filter groups are walked inside a team -- REDUCE launches of large problems --, mgroups == 1)
inline SegPlan plan_seg(const SearchInputs &in, int segl, int mode, int dc, int nfilters, int nslots, int mpb_want, bool inner_groups = false) {
    const SegGeom g = seg_geom(segl);
    SegPlan p;
    p.nsg = nslots >= 64 ? 8 : 1;
    // L = 256 runs three workgroups per CU only while a workgroup's LDS stays under 53 KiB: 8 filters per pass
    // (the wave-local 2048-point kernel keeps two workgroups per CU only while a workgroup's LDS stays under 80 KiB: 8 per pass)
    // (so does the 8192-point kernel: its one team per CU has 157 KiB with 8 filters per pass)
    int mpb = mpb_want > 0 ? mpb_want : ((segl <= 8 || segl == 13 || seg_ppl(1 << segl) == 32) ? 8 : SEG_MPB_MAX);
    if (mpb > seg_mpb_cap(segl)) mpb = seg_mpb_cap(segl);
    if (mpb > nfilters) mpb = nfilters;
    p.mgroups = (nfilters + mpb - 1) / mpb;
    p.mpb = (nfilters + p.mgroups - 1) / p.mgroups;   // balanced
    p.igroups = 1;
    // Workgroups in the grid per CU.  More than are resident at once (3 / 2 per CU): the surplus is dealt out as workgroups
    // retire, which evens out CUs that finish at different times.  Measured at C2, L = 256, settled clock, quiet host
    // (tools/seg_probe.py): 8 per CU 1.615 ms, 12: 1.615, 16: 1.613, 24: 1.604, 32: 1.596, 48: 1.595 -- about 1 %.  (Round 2's
    // table here -- 12: 1.90, 16: 1.71, 32: 1.655 "on an uneven device" -- was mostly the probe: its first variant ran in the
    // clock ramp after the handle was built.)  Small blocks are unaffected (the grid never has more teams than (bin, slot) units).
    const int wpc = in.seg_wpc > 0 ? in.seg_wpc : 32;
    // workgroups per group: wpc 256-thread workgroups' worth of teams per CU, over the device's CUs
    const int teams = wpc * in.num_cus * 256 / g.TEAM;         // teams in the whole grid
    int wpg = teams / g.TPW / p.nsg;
    if (wpg < 1) wpg = 1;
    // never more teams than (bin, slot) units in a group
    const long long units = (long long)dc * ((nslots + p.nsg - 1) / p.nsg);
    while (wpg > 1 && (long long)wpg * g.TPW > units) wpg >>= 1;
    // Several filter groups and plenty of (bin, slot) units: a team walks the groups itself on ONE forward transform per
    // segment instead of a workgroup per group each repeating it (1 of 18 transforms of the BPSK bank).  REDUCE launches only.
    if (inner_groups && segl <= 8 && p.mgroups > 1 && units >= 4LL * wpg * g.TPW) {      // (the 256-point kernel only: seg_kernels.hpp)
        p.igroups = p.mgroups;
        p.mgroups = 1;
    }
    p.wpg = wpg;
    // bsplit * ssplit = wpg * TPW teams; barrier teams of one workgroup must share the Doppler stream.
    // Of all factorisations take the one whose busiest team has the least (bins x slots) to do;
    // ties go to more Doppler streams (fewer partial-sum columns).
    const int tg = g.wave_sync ? wpg * g.TPW : wpg;
    const int glen = (nslots + p.nsg - 1) / p.nsg;
    int bs = 1;
    long long best = -1;
    for (int d = 1; d <= tg; ++d) {
        if (tg % d) continue;
        const int ss = g.wave_sync ? tg / d : (wpg / d) * g.TPW;
        const long long work = (long long)((dc + d - 1) / d) * ((glen + ss - 1) / ss);
        if (best < 0 || work <= best) {
            best = work;
            bs = d;
        }
    }
    p.bsplit = bs;
    p.ssplit = g.wave_sync ? tg / bs : (wpg / bs) * g.TPW;
    p.grid = p.nsg * p.mgroups * p.wpg;
    p.lds_bytes = seg_lds_bytes(segl, mode, p.mpb);
    return p;
}

// slots whose segments are all complete (branch-free kernel) and the rest (masked kernel)
inline void seg_slots(int N, const Segments &sg, int *full, int *total) {
    const SegGeom g = seg_geom(sg.segl);
    const int qfull = N / sg.V;                    // complete segments
    *full = qfull / g.CT;
    *total = (sg.Q + g.CT - 1) / g.CT;
}

// the matched-filter pass of nb blocks (SEG_STORE; demod_enqueue in bank_flight_api.hpp)
inline SegPlan plan_store(const SearchInputs &in, const Segments &sg, int nb) {
    int nfull, ntotal;
    seg_slots(in.N, sg, &nfull, &ntotal);
    return plan_seg(in, sg.segl, SEG_STORE, nb, in.M, ntotal, in.M <= SEG_MPB_MAX ? in.M : 4);
}

// ---- the search with the shift on the filter side (seg_kernels.hpp, segf_body) ------------------------------------------------------
// The instantiations of k_segf<L, PV, SUMQ> and k_seg<L, SEG_REDUCE, PV>: PV = seg_ppl(L) / 2 + I, I over SegSlots<L>.  Their dynamic LDS
// at `rows` filters per bin, and that of k_segw<SEGW_PV, SEGW_KT>, are stated here for the attributes and the launches.
template <int L>
using SegSlots = std::make_integer_sequence<int, seg_ppl(L) / 2 + 1>;
template <int L>
constexpr int segf_lds_bytes(int rows) {
    return (int)(SegCfg<L>::LDS_ELEMS * sizeof(cf) + (size_t)(SegCfg<L>::BLOCK / 64) * rows * SEG_ACC_STRIDE * sizeof(float));
}
constexpr int segf_rows_cap(int L) { return L == 2048 ? 8 : SEG_MPB_MAX; }
constexpr int SEGW_PV = 13, SEGW_KT = 3;      // the instantiated shape of the matrix-core form
constexpr int segw_lds_bytes() { return (int)SegWCfg<SEGW_PV, SEGW_KT>::lds_bytes(); }
// The SUMQ variant k_segf<L, pv, .> runs: 2 = the Parseval half of the complement form once per bin AND the filter rows summed in
// registers (qs: a SUM_ALL search with its table of sum |G|^2; presum: every row counted equally), 1 = the former alone, 0 = neither.
template <int L, int... I>
constexpr int segf_sumq(int pv, bool qs, bool presum, std::integer_sequence<int, I...>) {
    constexpr int P0 = seg_ppl(L) / 2;
    const bool one = qs && ((pv == P0 + I && segf_has_sumq<L, P0 + I>()) || ...);
    return one && presum && ((pv == P0 + I && segf_has_presum<L, P0 + I>()) || ...) ? 2 : one;
}

// K-steps of the matrix-core form of the search, 0 where it does not run: 256-point segments, SUM_ALL searches whose rows k_finalize
// counts equally (segf_body's SUMQ = 2 form), one 16-column tile per bin (MU <= 8) and the instantiated shape -- 13 valid register
// slots and at most three K-steps of 16 taps, which is 34 ... 48 taps (the 8-filter GMSK / FSK banks): seg_valid leaves 33 taps 14 valid
// slots, and 49 taps, which still have 13, need a fourth K-step.  The BPSK bank (80 taps, 16 rows) keeps segf_body.
// (tests/seg_model.py, wrap_form, restates this; tests/test_gpu_wrap_sweep.py holds the device to it at 33 | 34 and 48 | 49 taps.)
// Blocks of 2^18 samples and more only: a single small block (2^15 ... 2^17 samples x 64 bins) gets one-bin rectangles from fsm_plan, and
// there the forward transform and the A fragments, built per (slot, bin) at one wave per SIMD, made the search slower than segf_body
// (bench.py --full, recv_b1_n17_d64: 607 against 763 Msamples/s).  The choice depends on the bank and the block length alone -- never on
// the number of bins, the rectangle or the grid -- so that a (block, shift) scores the same bits from any handle, shard, tuning or batch.
inline int wrap_kt(const SearchInputs &in, const Segments &sg, bool presum, int MU) {
    if (!in.wrap_mfma || sg.segl != 8 || in.N < (1 << 18) || !in.sum_all || !MFB_SEG_SUMQ || MU > 8) return 0;
    if (!presum || !segf_has_presum<256, SEGW_PV>() || sg.V != SEGW_PV * SegCfg<256>::NT) return 0;
    return (in.T > 32 && in.T <= 16 * SEGW_KT) ? SEGW_KT : 0;
}
// A wave's rectangle (bins x slots) and what a group of the grid is.  The forward transform is shared by fb bins -- 1 / (fb MU) of
// the inverse work --; small rectangles keep the grid over-subscribed (the surplus evens out CUs that finish at different times, as
// in plan_seg).  Measured (profiles/r06_fft_ops.md): 128 (bin, filter) transforms of 256 points per forward transform -- 16 bins
// of the 8-filter banks, 8 of the BPSK bank's 16 --, 64 of 2048 points.  Groups (blockIdx % 8 = XCD): an eighth of the BINS when
// there are enough of them -- every XCD then keeps its share of the per-bin spectra in its L2 (C3: +4.5 %; the 2048-point kernel,
// 32 MiB of spectra at 256 bins: 2.09 against 2.49 ms) and the samples stream through all of them --, else an eighth of the slots.
//
// The matrix-core form (k_segw) plans for itself.  A wave of it pays a slot's prologue -- samples, window, forward transform and the
// 160 fragment registers, the matrix pipe idle and nothing else on the SIMD -- once per rectangle, so its rectangle is the group's
// whole share of bins, in equal chunks of at most SEGW_FB (256 bins: 32, one chunk; 1024: four chunks of 32), and SEGW_FS slots
// (measured, profiles/r12_wrap_slots.md: C2 2055 Msamples/s at 16 x 1, 2295 at 32 x 1, 2316 at 32 x 2, 2310 ... 2323 at 32 x 5, 2273
// at 32 x 10, one launch round with nothing to even out).  It holds one wave per SIMD, not three: its small-launch bound is a wave for
// every SIMD, reached by giving up slots per wave first, which cost nothing, and bins only then.
//
// The wide plan of k_segw (profiles/r14_wrap_wide.md): chunks of at most SEGW_WIDE_FB = 64 bins, so that a slot's fragments are built
// by half as many waves (C3 1.068x, 384 bins 1.07x, C2 1.03x on top of the pick's copy).  Its groups are always groups of BINS, with
// the four waves of a workgroup on four slots of the same bins: they fetch the same 7 KiB of tables a bin (Wb 6 KiB, Qs 1 KiB) at
// about the same time, so three of four fetches end in the CU's vector cache.  Over groups of slots the four waves are the four
// chunks of one slot, every fetch goes to the L2 (measured at C2: 20.7 M L2 hits a launch against 7.0 M) and 64 bins gain 1 %
// instead of 4.  So where an eighth of the bins does not fill a chunk and a quarter does (Dtot <= 256), the grid has FOUR groups,
// each on a pair of XCDs (blockIdx % 4); from there on eight.  Under 128 bins the plan above stands.  A rectangle twice as long needs
// twice the rounds to even out CUs that finish at different times, so the wide plan applies only where a launch of one-slot
// rectangles has four waves for every SIMD, and it takes the most slots a wave (5 ... 1) that keep those four rounds (C2: 5040 waves
// of 64 x 1; C3: 5040 of 64 x 4).  Anything smaller gets the plan above, unchanged.  Which form runs does not depend on the
// rectangle or the groups (wrap_kt).
//
// ok NEVER depends on nb: what is decided with one block (the tables built ahead, mfb_get_search_info) holds for the batch launched.
struct FsmPlan {
    bool ok;
    int nsg, gbins, fb, fs, nbc, nsc;
};
constexpr int SEGW_FB = 32, SEGW_FS = 5;
constexpr int SEGW_WIDE_FB = 64, SEGW_WIDE_ROUNDS = 4;
// segw: the launch takes k_segw -- the bank, the basis and the block length decide (wrap_kt), nothing else
inline FsmPlan fsm_plan(const SearchInputs &in, int segl, bool segw, int MU, int nfull, int nb) {
    const int env_gb = in.group;
    FsmPlan p = {};
    const bool w32 = segl == 11;
    p.nsg = nfull >= 64 ? 8 : 1;
    const int per_fwd = w32 ? 64 : 128;
    const bool fb_set = in.rect_fb > 0, fs_set = in.rect_fs > 0;
    int fb = fb_set ? in.rect_fb : (per_fwd / MU > 2 ? per_fwd / MU : 2);
    int fs = fs_set ? in.rect_fs : (segw ? SEGW_FS : 1);
    if (segw && !fb_set && env_gb < 0 && p.nsg > 1 && in.Dtot >= 4 * SEGW_FB) {
        // the wide plan, where the launch is long enough for it
        const int wnsg = in.Dtot <= 4 * SEGW_WIDE_FB ? 4 : 8;
        const int share = (in.Dtot + wnsg - 1) / wnsg;
        const int chunks = (share + SEGW_WIDE_FB - 1) / SEGW_WIDE_FB;
        const long long want = (long long)SEGW_WIDE_ROUNDS * 4 * in.num_cus;
        auto wwaves = [&](int s) { return (long long)nb * wnsg * chunks * ((nfull + s - 1) / s); };
        if (wwaves(1) >= want) {
            if (fs > nfull) fs = nfull;
            while (!fs_set && fs > 1 && wwaves(fs) < want) --fs;
            p.nsg = wnsg;
            p.gbins = 1;
            p.fb = (share + chunks - 1) / chunks;
            p.fs = fs;
            p.nbc = (share + p.fb - 1) / p.fb;
            p.nsc = (nfull + fs - 1) / fs;
            p.ok = true;
            return p;
        }
    }
    if (fb > in.Dtot) fb = in.Dtot;
    p.gbins = env_gb >= 0 ? (env_gb != 0) : (p.nsg > 1 && in.Dtot >= p.nsg * fb ? 1 : 0);
    if (p.gbins && in.Dtot < p.nsg) p.gbins = 0;
    if (w32 && !p.gbins && p.nsg > 1 && env_gb < 0) {
        // the long kernel's spectra (16 KiB per (bin, filter)) must stay in an L2: fewer bins per rectangle, or not this kernel
        fb = in.Dtot / p.nsg;
        if (fb < 1) return p;
        p.gbins = 1;
    }
    const int glen = p.gbins ? nfull : (nfull + p.nsg - 1) / p.nsg;
    const int gblen = p.gbins ? (in.Dtot + p.nsg - 1) / p.nsg : in.Dtot;
    if (segw && !fb_set) {
        const int chunks = (gblen + SEGW_FB - 1) / SEGW_FB;
        fb = (gblen + chunks - 1) / chunks;
    }
    if (fs > glen) fs = glen;
    if (fb > gblen) fb = gblen;
    if (fb < 1 || fs < 1) return p;
    // Small problems (one block of 2^15 samples x 64 bins: 2496 (bin, slot) units) must not be folded into a few long waves: the
    // rectangle shrinks until the launch has twice the waves the device holds at once -- at one bin per rectangle the forward
    // transform is no longer shared, and what is left of the gain is the mixing multiply (measured: bench.py's one-block loop at
    // 2^15 x 64 fell from 250 to 155 Msamples/s with 16-bin rectangles: 156 waves on 1024 SIMDs)
    auto waves = [&] { return (long long)nb * p.nsg * ((gblen + fb - 1) / fb) * ((glen + fs - 1) / fs); };
    if (segw) {
        const long long want = 4LL * in.num_cus;
        while (!fs_set && fs > 1 && waves() < want) fs = (fs + 1) >> 1;
        while (!fb_set && fb > 1 && waves() < want) fb = (fb + 1) >> 1;
    } else if (!fb_set) {
        const long long want = 2LL * in.num_cus * 4 * (w32 ? 2 : 3);
        while (fb > 1 && waves() < want) fb >>= 1;
    }
    p.fb = fb;
    p.fs = fs;
    p.nbc = (gblen + fb - 1) / fb;
    p.nsc = (glen + fs - 1) / fs;
    p.ok = true;
    return p;
}

// ---- one search, decided once --------------------------------------------------------------------------------------------------------
// The segment-path search of nb blocks: ONE main launch over the complete slots of all bins (nothing of length N is written, so there
// is nothing to chunk), a second, tiny launch of the masked instantiation over the slots that hold incomplete segments, k_finalize.
// The plan is the single answer to "what will the next search launch": launched, reported and built for as it stands.
inline SearchPlan plan_search(const SearchInputs &in, const Segments &sg, int nb) {
    SearchPlan p = {};
    p.path = sg.path, p.segl = sg.segl, p.V = sg.V, p.T = sg.T, p.Q = sg.Q, p.basis = sg.basis;
    if (sg.path != MFB_PATH_SEGMENT) return p;
    const bool span = sg.basis == MFB_BASIS_SPAN;
    const int MU = span ? in.MB : in.MU;     // filters transformed per bin
    const int dc = nb * in.Dtot;             // Doppler streams of the launch
    const SegGeom g = seg_geom(sg.segl);
    seg_slots(in.N, sg, &p.nfull, &p.ntotal);
    p.rows = MU, p.pv = sg.V / g.NT;
    // one partial per (bin, filter, slot, wave of the team): the index depends on the slot alone (seg_kernels.hpp)
    p.parts = p.ntotal * g.WPT;
    p.presum = span || in.uniform_mult;      // every unique row is counted equally
    // the tail is a handful of units: spread the filters too (2 per pass) so that it is short
    if (p.ntotal > p.nfull) p.tail = plan_seg(in, sg.segl, SEG_REDUCE, dc, MU, p.ntotal - p.nfull, in.seg_mpb > 0 && in.seg_mpb < 2 ? in.seg_mpb : 2);
    if (p.nfull == 0) return p;
    // 256-point segments: the shift on the filter side -- one forward transform per segment for all bins (segf_body)
    // (the wave-local 2048-point kernel too: 8 filters per pass there, and per-bin spectra of 16 KiB per (bin, filter) -- up to 256 MiB)
    const bool fsm_l = sg.segl == 8 || (sg.segl == 11 && MFB_SEG_W32 && MU <= 8 && (size_t)in.Dtot * MU * 16384 <= ((size_t)256 << 20));
    const int wkt = wrap_kt(in, sg, p.presum, MU);
    FsmPlan fp;
    if (fsm_l && in.fsm && MFB_FFT_FUSED && MU <= SEG_MPB_MAX && in.shifts_known && (fp = fsm_plan(in, sg.segl, wkt != 0, MU, p.nfull, nb)).ok) {
        const bool qs = in.sum_all && MFB_SEG_SUMQ;
        p.form = sg.segl == 11 ? SEARCH_SEGF2048 : (wkt ? SEARCH_SEGW : SEARCH_SEGF256), p.wrap_kt = wkt;
        p.sumq = sg.segl == 11 ? segf_sumq<2048>(p.pv, qs, p.presum, SegSlots<2048>{}) : segf_sumq<256>(p.pv, qs, p.presum, SegSlots<256>{});
        p.nsg = fp.nsg, p.gbins = fp.gbins, p.fb = fp.fb, p.fs = fp.fs, p.nbc = fp.nbc, p.nsc = fp.nsc;
        const int wpb = SegCfg<256>::BLOCK / 64;
        static_assert(SegCfg<256>::BLOCK == SegCfg<2048>::BLOCK || !MFB_SEG_W32, "four independent waves per workgroup");
        p.grid = p.nsg * (int)(((long long)nb * p.nbc * p.nsc + wpb - 1) / wpb);
        p.lds_bytes = p.form == SEARCH_SEGF2048 ? segf_lds_bytes<2048>(MU) : (p.form == SEARCH_SEGW ? segw_lds_bytes() : segf_lds_bytes<256>(MU));
        p.need_tables = 1, p.need_rows = MU, p.need_span = span, p.need_segl = sg.segl, p.need_wkt = wkt;      // (fsm_prepare builds them)
    } else {
        p.form = SEARCH_SEG;
        p.main_seg = plan_seg(in, sg.segl, SEG_REDUCE, dc, MU, p.nfull, in.seg_mpb, true);
    }
    return p;
}
