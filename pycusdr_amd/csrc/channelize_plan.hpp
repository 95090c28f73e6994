// channelize_plan.hpp -- the channeliser's launch plan: the ONE statement of its limits, of the arithmetic that sizes a workgroup's
// LDS image, and of what a plan of each kind launches (mfb_channelizer_* in channelize_api.hpp and mfb_synthesizer_* in synthesize_uniform_api.hpp; the kernels are
// channelize_kernels.hpp, channelize_rational_kernels.hpp, channelize_uniform_kernels.hpp, channelize_uniform_rational_kernels.hpp,
// channelize_survey_kernels.hpp and synthesize_uniform_kernels.hpp, which include this for the limits their argument structs and
// launch bounds use).  Host only and
// free of HIP, so a plain C++ compiler builds it (tests/csrc/channelize_plan_print.cpp and synthesize_plan_print.cpp;
// tests/golden/channelize_plans.json was recorded from the helpers below before ChzGeom was built on them).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cmath>

// ---- limits
#define CHZ_MAX_CHANNELS 16
#define CHZ_MAX_DECIM 64
#define CHZ_MAX_TAPS 1024
#define CHZ_MAX_THREADS 256
#define CHZ_LDS_BUDGET (48 * 1024)   // bytes of LDS a workgroup may take: three workgroups per CU at the least
#define CHZ_MAX_IN (1 << 24)         // samples per call
#define CHZ_MAX_OUT (1 << 22)        // outputs per channel and call
#define CHZR_MAX_INTERP 32
#define CHU_THREADS 256
#define CHU_MAX_BINS 256
#define CHU_MAX_TAPS 4096
#define CHU_LDS_BUDGET (64 * 1024)
#define CHU_MAX_SET (1 << 26)        // complex64 per output set
#define CHUS_MIN_LOG2 2
#define CHUS_MAX_LOG2 16
#define CHUS_MAX_TABLE (1 << 22)     // (cell, bin) entries per call
#define CHUS_SCRATCH 256             // floats behind the uniform kernel's LDS
#define CHZ_CF_BYTES 8               // sizeof(float2): one staged sample, one image word
#define CHSY_MAX_FRAMES 4096         // placements per call of the synthesiser
#define CHSY_MAX_OUT (1 << 24)       // wide outputs per call
#define CHSY_MAX_SOURCE (1 << 26)    // complex64 of a source copied in
#define CHSY_MAX_TILE 128            // input frames a workgroup makes outputs for, at the most

// ---- the geometry of each kernel (the rules are in the kernel headers' comments)
// rows of the LDS image for a workgroup of `threads` lanes: ceil(span / D), made odd
static inline int chz_row_len(int threads, int D, int T) {
    const int span = (threads - 1) * D + T;
    return ((span + D - 1) / D) | 1;
}

// the largest workgroup whose image fits the budget (64 lanes always do: 64 * 81 * 8 bytes at D = 64, T = 1024)
static inline int chz_threads(int D, int T) {
    for (int w = CHZ_MAX_THREADS; w > 64; w >>= 1)
        if ((size_t)D * chz_row_len(w, D, T) * CHZ_CF_BYTES <= (size_t)CHZ_LDS_BUDGET) return w;
    return 64;
}

static inline int chzr_branch_taps(int U, int T) { return (T + U - 1) / U; }
static inline int chzr_span(int threads, int U, int D, int T) { return chzr_branch_taps(U, T) - 1 + threads * D; }
static inline int chzr_row_len(int threads, int U, int D, int T) { return ((chzr_span(threads, U, D, T) + D - 1) / D) | 1; }
// the largest workgroup whose image fits the budget (64 lanes always do: 64 * 81 * 8 bytes at D = 64, Tb = 1024)
static inline int chzr_threads(int U, int D, int T) {
    for (int w = CHZ_MAX_THREADS; w > 64; w >>= 1)
        if ((size_t)D * chzr_row_len(w, U, D, T) * CHZ_CF_BYTES <= (size_t)CHZ_LDS_BUDGET) return w;
    return 64;
}

static inline size_t chu_lds_bytes(int M, int D, int T, int F) {
    return ((size_t)(F - 1) * D + T + (size_t)F * (M + 1) + M) * CHZ_CF_BYTES;
}

// frames per workgroup (channelize_uniform_kernels.hpp has the rule)
static inline int chu_frames(int M, int D, int T) {
    const int step = 256 / M > 16 ? 256 / M : 16;
    int F = 4096 / M > 128 ? 128 : 4096 / M;
    while (F > step && chu_lds_bytes(M, D, T, F) > (size_t)CHU_LDS_BUDGET) F -= step;
    while (F * M > 256 && chu_lds_bytes(M, D, T, F) > (size_t)CHU_LDS_BUDGET) F >>= 1;
    return F;
}

// A rational plan on the raster (channelize_uniform_rational_kernels.hpp): F consecutive frames read the positions
// q(m0) - (Tb - 1) .. q(m0 + F - 1), q(m) = (m D) div U, and q(m0 + F - 1) - q(m0) <= ((F - 1) D + U - 1) div U, reached where
// (m0 D) mod U = U - 1.  With U = 1 the span, the bytes and the frames are chu_lds_bytes' and chu_frames'.
static inline int chur_span(int U, int D, int T, int F) { return chzr_branch_taps(U, T) + (int)(((int64_t)(F - 1) * D + U - 1) / U); }
static inline size_t chur_lds_bytes(int M, int U, int D, int T, int F) {
    return ((size_t)chur_span(U, D, T, F) + (size_t)F * (M + 1) + M) * CHZ_CF_BYTES;
}

// frames per workgroup: chu_frames' rule with that span.  F = 1 at M = 256 always fits: (4096 + 257 + 256) * 8 bytes.
static inline int chur_frames(int M, int U, int D, int T) {
    const int step = 256 / M > 16 ? 256 / M : 16;
    int F = 4096 / M > 128 ? 128 : 4096 / M;
    while (F > step && chur_lds_bytes(M, U, D, T, F) > (size_t)CHU_LDS_BUDGET) F -= step;
    while (F * M > 256 && chur_lds_bytes(M, U, D, T, F) > (size_t)CHU_LDS_BUDGET) F >>= 1;
    return F;
}

// the synthesiser (synthesize_uniform_kernels.hpp): the image of the F + J - 1 input frames that the outputs of F frames read,
// J = ceil(T / I), rows of M + 1 words; the twiddle table; the taps
static inline int chsy_rows(int I, int T, int F) { return F + chzr_branch_taps(I, T) - 1; }
static inline size_t chsy_lds_bytes(int M, int I, int T, int F) {
    return ((size_t)chsy_rows(I, T, F) * (M + 1) + M) * CHZ_CF_BYTES + (size_t)T * sizeof(float);
}

// Frames per workgroup of the synthesiser: the largest F <= CHSY_MAX_TILE whose image fits CHU_LDS_BUDGET (a larger tile repeats
// fewer transforms, (J - 1) / F of them; beyond 128 frames that share is small and the grid of a short call would thin out).
// 0: not even F = 1 fits, the plan is refused.  J <= 17 always fits: (17 * 257 + 256) * 8 + 4096 * 4 = 53384 bytes at M = 256.
static inline int chsy_frames(int M, int I, int T) {
    int F = CHSY_MAX_TILE;
    while (F > 0 && chsy_lds_bytes(M, I, T, F) > (size_t)CHU_LDS_BUDGET) --F;
    return F;
}

static inline size_t chus_lds_bytes(int M, int D, int T, int Fs) { return chu_lds_bytes(M, D, T, Fs) + CHUS_SCRATCH * sizeof(float); }

// frames per workgroup of a survey launch
static inline int chus_frames(int M, int D, int T) {
    const int F = chu_frames(M, D, T);
    int Fs = 1;
    while (2 * Fs <= F) Fs <<= 1;
    while (Fs * M > 256 && chus_lds_bytes(M, D, T, Fs) > (size_t)CHU_LDS_BUDGET) Fs >>= 1;
    return Fs;
}

// ---- what a plan launches
// k_chz, k_chzr, k_chu, k_chus, k_chsy, k_chur (appended: recorded plans keep their values)
enum ChzKind { CHZ_INTEGER = 0, CHZ_RATIONAL = 1, CHZ_UNIFORM = 2, CHZ_SURVEY = 3, CHZ_SYNTHESIS = 4, CHZ_UNIFORM_RATIONAL = 5 };

struct ChzGeom {
    int kind;
    int U, D, T;           // interpolation (1 unless rational; the synthesiser's I), decimation (the synthesiser's is 1), taps
    int Tb;                // ceil(T / U): the taps of the longest branch
    int M;                 // the raster's bins (uniform, uniform rational, survey, synthesis); 0 otherwise
    int threads;           // lanes of a workgroup
    int tile;              // outputs per workgroup: threads, U threads, F or Fs by kind; synthesis: the F input frames whose F I
                           // outputs a workgroup makes, 0 where the plan does not fit
    int L;                 // float2 per LDS row (integer, rational); 0 otherwise
    int S;                 // staged positions of a rational plan, on the raster or not; 0 otherwise
    size_t lds_bytes;      // dynamic LDS of the launch
};

// U is read for a rational plan, on the raster or not, and for a synthesis (its I, with D = 1), M for a plan on the raster, its
// survey or a synthesis; the limits are the caller's to check
static inline ChzGeom chz_geom(int kind, int U, int D, int T, int M) {
    ChzGeom g = {};
    g.kind = kind;
    g.U = (kind == CHZ_RATIONAL || kind == CHZ_SYNTHESIS || kind == CHZ_UNIFORM_RATIONAL) ? U : 1;
    g.D = D;
    g.T = T;
    g.Tb = chzr_branch_taps(g.U, T);
    switch (kind) {
        case CHZ_INTEGER:
            g.threads = g.tile = chz_threads(D, T);
            g.L = chz_row_len(g.threads, D, T);
            g.lds_bytes = (size_t)D * g.L * CHZ_CF_BYTES;
            break;
        case CHZ_RATIONAL:
            g.threads = chzr_threads(U, D, T);
            g.tile = U * g.threads;
            g.L = chzr_row_len(g.threads, U, D, T);
            g.S = chzr_span(g.threads, U, D, T);
            g.lds_bytes = (size_t)D * g.L * CHZ_CF_BYTES;
            break;
        case CHZ_UNIFORM:
            g.M = M;
            g.threads = CHU_THREADS;
            g.tile = chu_frames(M, D, T);
            g.lds_bytes = chu_lds_bytes(M, D, T, g.tile);
            break;
        case CHZ_UNIFORM_RATIONAL:
            g.M = M;
            g.threads = CHU_THREADS;
            g.tile = chur_frames(M, U, D, T);
            g.S = chur_span(U, D, T, g.tile);
            g.lds_bytes = chur_lds_bytes(M, U, D, T, g.tile);
            break;
        case CHZ_SYNTHESIS:
            g.M = M;
            g.threads = CHU_THREADS;
            g.tile = chsy_frames(M, g.U, T);
            g.lds_bytes = g.tile ? chsy_lds_bytes(M, g.U, T, g.tile) : 0;
            break;
        default:
            g.M = M;
            g.threads = CHU_THREADS;
            g.tile = chus_frames(M, D, T);
            g.lds_bytes = chus_lds_bytes(M, D, T, g.tile);
            break;
    }
    return g;
}

// workgroups of a call of out_count outputs (every kind but a synthesis tiles the outputs: tile is threads, U threads, F or Fs)
static inline unsigned chz_grid(const ChzGeom &g, int out_count) { return (unsigned)((out_count + g.tile - 1) / g.tile); }

// A synthesis tiles the input frames, not the outputs: the wide outputs [out_base, out_base + out_count) belong to the frames
// out_base div I .. (out_base + out_count - 1) div I, workgroup g taking F of them from (out_base div I) + g F on.
static inline void chsy_frame_span(const ChzGeom &g, int64_t out_base, int out_count, int64_t *first, int64_t *last) {
    *first = out_base / g.U;
    *last = (out_base + out_count - 1) / g.U;
}
static inline unsigned chsy_grid(const ChzGeom &g, int64_t out_base, int out_count) {
    int64_t first = 0, last = 0;
    chsy_frame_span(g, out_base, out_count, &first, &last);
    return (unsigned)((last - first + g.tile) / g.tile);
}

// Every input that the outputs [out_base, out_base + out_count) read lies in [*first, *last]; *first may be negative, positions
// below 0 read as zero.  A rational plan, on the raster or not: [q(out_base) - (Tb - 1), q(out_base + out_count - 1)] with
// q(m) = (m D) div U, one sample generous for short branches.
static inline void chz_input_span(const ChzGeom &g, int64_t out_base, int out_count, int64_t *first, int64_t *last) {
    *first = out_base * g.D / g.U - (g.Tb - 1);
    *last = (out_base + out_count - 1) * g.D / g.U;
}

// ---- the survey's tables, sv the CHZ_SURVEY geometry of the plan
// frames per partial: a whole cell, or the subtree of one that a workgroup holds
static inline int chus_chunk(const ChzGeom &sv, int cell_frames) { return cell_frames < sv.tile ? cell_frames : sv.tile; }

struct ChusTables {
    int64_t cells;         // of the longest call: max_out outputs, M out_count <= CHU_MAX_SET, M out_count / L <= CHUS_MAX_TABLE
    int64_t chunks;        // partials per bin of that call
    int words;             // mask words per cell
};

static inline ChusTables chus_tables(const ChzGeom &sv, int cell_frames, int max_out) {
    ChusTables t;
    const int64_t most = (int64_t)max_out < (int64_t)CHU_MAX_SET / sv.M ? (int64_t)max_out : (int64_t)CHU_MAX_SET / sv.M;
    t.cells = most / cell_frames;
    if (t.cells > CHUS_MAX_TABLE / sv.M) t.cells = CHUS_MAX_TABLE / sv.M;
    t.chunks = t.cells * (cell_frames / chus_chunk(sv, cell_frames));
    t.words = (sv.M + 31) / 32;
    return t;
}

// ---- a plan's scalar arguments (the formats are MFB_SAMPLES_CF32 / _SC16 / _SC8 of include/mfbank.h)
static inline bool chz_format_ok(int fmt) { return fmt == 0 || fmt == 1 || fmt == 2; }

// The scale a plan runs with: 1 for complex64; for integers sample_scale, or 2^-15 (sc16) / 2^-7 (sc8) where that is 0.
// false: scale_ok (chan_scale_ok of channel_api.hpp: a power of two within 2^-100 .. 2^98) refuses it.
static inline bool chz_plan_scale(int fmt, float sample_scale, bool (*scale_ok)(float), float *scale) {
    *scale = 1.0f;
    if (fmt == 0) return true;
    *scale = sample_scale == 0.0f ? (fmt == 1 ? 0x1p-15f : 0x1p-7f) : sample_scale;
    return scale_ok(*scale);
}

static inline bool chz_taps_finite(const float *taps, int ntaps) {
    for (int t = 0; t < ntaps; ++t)
        if (!std::isfinite(taps[t])) return false;
    return true;
}

// gcd(U, D) == 1, for U, D >= 1
static inline bool chzr_coprime(int U, int D) {
    while (U) {
        const int r = D % U;
        D = U;
        U = r;
    }
    return D == 1;
}
