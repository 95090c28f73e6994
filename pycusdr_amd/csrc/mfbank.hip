// mfbank.hip -- hand-written gfx950 kernels + C ABI for the Doppler matched-filter bank.
//
// Data layout in HBM (N = N1*N2 samples per block, D Doppler bins, M matched filters):
//   d_x     complex64 [N]        time-domain block (or caller's device pointer)
//   d_X     complex64 [N]        spectrum, natural order
//   d_masks complex64 [M][N]     filter bank as protocol.get_filter returns it (row-major)
//   d_Z     complex64 [Dc*MU][N1][N2] intermediate of the two-pass inverse FFT for ONE chunk of
//                                Dc Doppler bins x MU unique filters: Z[row][n1][k2], already multiplied
//                                by the inter-pass twiddle W_N^(k2*n1).  Never holds the D*M*N cube.
//   d_part  float32 [D][MU][PARTS] per-workgroup partial |.|^2 sums (fixed-order second reduction,
//                                no float atomics -> bit-reproducible).  Searches that sum a bin's rows in
//                                registers (k_segw, k_segf's SUMQ = 2 form) write row 0 of the complete slots only:
//                                rows >= 1 are defined from the masked tail's first partial on, stale below it, and
//                                k_finalize is told so (presum, tail0)
//   d_sum   float32 [D][M]       doppSum, same meaning/layout as the reference's GPU_bufDoppSum
//   d_xc    complex64 [M][N]     matched-filter outputs at the chosen shift (natural order)
//
// Two-pass inverse FFT of length N = N1*N2 with input index k = N2*k1 + k2 and output index
// n = n1 + N1*n2:
//   pass 1 (k_pass1): for 16 adjacent k2 ("tile"), all k1: load X[(k+shift) mod N]*mask[m][k] on the
//           fly (128-byte coalesced segments), N1-point FFT over k1 in registers+LDS, multiply
//           by W_N^(k2*n1), store Z[n1][k2] (128-byte segments).
//   pass 2 (k_pass2): for every n1: N2-point FFT over k2 of the contiguous row Z[n1][:], then either
//           reduce |y|^2 in registers -> wave -> workgroup (Doppler search; the time-domain rows
//           are never written), or write the row back in place and let k_transpose produce
//           y[n1 + N1*n2] (demodulation / forward FFT).
//
// Short filters (every shipped protocol) take the single-pass overlap-save path instead (seg_kernels.hpp):
// no intermediate at all; the two-pass path below stays as the fallback for filters without a short
// impulse response and for blocks too small to segment, and serves the plain forward transforms.
//
// This file keeps the bank (mfb_ctx and everything that serves it).  The six side handles -- sync finder, combiner, modulator,
// channel, channeliser, synthesiser -- have their host side in sync_api.hpp, combine_api.hpp, mod_api.hpp, channel_api.hpp,
// channelize_api.hpp and synthesize_uniform_api.hpp, included below where that code stood (one translation unit, as before);
// what they share is stage_handle.hpp, what they share with the bank mfb_common.hpp.
//
// Reference semantics reproduced (file:line in the reference tree, pyCuSDR/):
//   shift-multiply  demodulator/cuda_kernels.cu:339-373, 174-185
//   |.|^2 / 2^18 row sums  cuda_kernels.cu:421-480      pick  cuda_kernels.cu:502-597
//   envelope        cuda_kernels.cu:191-205             rate/phase  cuda_kernels.cu:236-320
//   centres         cuda_kernels.cu:78-146
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/mfbank.h"
#include "fft_core.hpp"
#include "filter_taps.hpp"
#include "seg_kernels.hpp"
#include "wrap_kernels.hpp"
#include "search_plan.hpp"
#include "twopass_kernels.hpp"
#include "small_kernels.hpp"
#include "sync_kernels.hpp"
#include "combine_kernels.hpp"
#include "mod_kernels.hpp"
#include "channel_kernels.hpp"
#include "channelize_kernels.hpp"
#include "channelize_rational_kernels.hpp"
#include "channelize_uniform_kernels.hpp"
#include "channelize_uniform_rational_kernels.hpp"
#include "synthesize_uniform_kernels.hpp"
#include "channelize_survey_kernels.hpp"
#include "energy_kernels.hpp"
#include "stream_kernels.hpp"
#include "clip_kernels.hpp"
#include "snr_kernels.hpp"
#include "unpack_kernels.hpp"
#include "hostcopy.hpp"
#include "hip_owned.hpp"
#include "mfb_common.hpp"
#include "stage_handle.hpp"
#include "record_layout.hpp"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct BlockFlight {      // one block -- or one batch of nb blocks -- between mfb_receive_block(s)_begin and _end
    bool active;
    int mode, nthreads, bcap, shift, op;
    int nb;               // 0: a single block (mfb_receive_block_begin); > 0: a batch (mfb_receive_blocks_begin)
    RecordLayout lay;     // where things sit inside a record; lay.bytes apart in the staging buffer (batches)
    unsigned long long seq;
    bool clip;            // the block(s) went through the peak clip (mfb_get_block_clips)
    bool dsnr;            // searched with mfb_set_device_snr on: the record holds the two window means (mfb_get_block_snr)
};

constexpr int WG_NB = 32;
struct BlockGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    mfb_block_params params;
    int nb;               // blocks of the batch the graph was recorded for (0: single block)
    unsigned long long epoch;
    bool seen, failed;
};

// Every buffer, event and library-made stream of a handle is an owner (hip_owned.hpp), and every member has an initialiser: adding one
// is one declaration here.  ~mfb_ctx releases them in reverse order of declaration, so the four streams, declared first, go last:
// behind every event recorded on them and every buffer their work used (mfb_destroy has waited for all four by then).
struct mfb_ctx {
    Stream own_stream, copy_stream, in_stream, s2;   // the handle's own; the spectrum mirror's; host-to-device copies of the block path; part 2 (below)
    hipStream_t stream = nullptr;                    // own_stream, or the caller's (mfb_set_stream): not owned
    int device = 0;
    int log2N = 0, N = 0, N1 = 0, N2 = 0, l1 = 0, l2 = 0, lo = 0;
    int D = 0, Doff = 0, Dtot = 0, M = 0, W = 0, sum_all = 0, cs_off = 0;
    int chunk = 0, mpb = 0, jsplit = 0;
    int MU = 0;           // unique filter rows (up to sign)
    bool chunk_auto = false;      // chunk still at its default (recomputed when the bank turns out to have duplicates)
    DevBuf<int> d_uniq, d_rep;    // [MU] bank row of each unique filter; [M] unique index of each filter
    int parts = 0, srb = 0;
    int num_cus = 0;      // compute units of the handle's device
    HostBuf<cf> h_in;     // pinned
    // page-locked landing zone of the small read-backs (pick, rate/phase, spectrum windows, symbol decisions): a
    // copy into pageable memory is staged by the runtime with a round trip of its own per copy
    HostBuf<uint8_t> h_back;
    size_t back_cap = 0;
    // the pick's own page-locked slot, 16 bytes, coherent: k_pick stores {two floats, the pick's number, a check word} there itself
    // (h_pick_dev: the slot as the device addresses it), so that no copy -- a blit kernel and its dispatch gap for 8 bytes -- stands
    // between the kernel and the host's read, and the host takes the pick when it arrives (read_pick); picks: picks asked for so far
    HostBuf<uint32_t> h_pick;
    u32x4 *h_pick_dev = nullptr;
    uint32_t picks = 0;
    // Host mirror of the spectrum for small blocks.  The reference keeps the spectrum in host-mapped memory and reads
    // its SNR windows straight from there (DB:456-457, 651-661); here the first mfb_get_spectrum on a handle turns on
    // an asynchronous copy of every new spectrum (own stream, beside the search), so that later window reads cost no
    // host-device round trip.  Blocks above MIRROR_MAX_N keep fetching windows on demand.
    HostBuf<cf> h_X;
    bool mirror = false, mirror_valid = false;
    Event ev_fft, ev_X;
    DevBuf<cf> d_x, d_X, d_masks, d_Z, d_xc, d_P;
    const cf *d_in = nullptr;  // current time-domain input (d_x or caller's device pointer): not owned
    DevBuf<float> d_env;
    DevBuf<int> d_shifts;
    DevBuf<cf> d_tw1, d_tw2, d_twLo, d_twHi;
    DevBuf<float> d_part, d_sum, d_res, d_cr;
    DevBuf<int> d_sym, d_cen;
    DevBuf<float> d_mag;
    int cap = 0;  // capacity of the centres buffers
    size_t z_rows = 0;  // rows allocated in d_Z
    bool have_filters = false, have_shifts = false, have_input = false, have_xc = false;
    Event t0, t1;
    bool prof = false;
    // single-pass overlap-save path (seg_kernels.hpp)
    int path_req = 0, segl_req = 0;   // requested: MFB_PATH_*, log2 L (0 = automatic)
    int path = 0, segl = 0;           // resolved
    int T = 0, win_start = 0, V = 0, Q = 0;   // taps, window start, valid outputs per segment, segments
    int seg_wpc = 0, seg_mpb = 0;     // workgroups per CU, filters per team pass (0 = automatic)
    DevBuf<cf> d_G, d_twL;
    int twL_len = 0;
    size_t part_cap = 0;              // floats allocated in d_part
    std::unique_ptr<taps::Bank> bank; // host copy of the taps (kept so that L can be changed)
    int basis_req = 0, basis = 0;     // MFB_BASIS_*: requested / in force
    int MB = 0;                       // filters of the span basis
    DevBuf<cf> d_Gb;                  // their segment spectra [MB][L] (slot-pair layout)
    int gb_l = 0;                     // segment length d_Gb was built for
    int search_mode = 0;              // MFB_SEARCH_*: transforms (default) or the opt-in spectral-energy shortcut
    DevBuf<float> d_pow, d_W;         // |X|^2 [N]; filter energy [R][N] (R = 1 under SUM_ALL_MASKS, else M)
    HostBuf<cf> h_in2;                // second page-locked input buffer (blocks in flight alternate between the two)
    DevBuf<cf> d_x2;                  // its device copy: the next block's samples arrive (own stream) while the current block is searched
    Event ev_h2d[2];                  // [input buffer]: the copy has landed
    Event ev_xfree[2];                // [input buffer]: the last block that read this device copy has been enqueued and finished
    HostBuf<uint8_t> h_blk[2];        // page-locked staging of the two block flights
    size_t blk_cap[2] = {};
    Event ev_blk[2];
    BlockFlight flight[2] = {};
    unsigned long long blk_seq = 0;
    BlockGraph bgraph[2][2] = {};     // [input buffer][slot]: the block's launches as a HIP graph
    unsigned long long epoch = 0;     // bumped by every change that invalidates them
    DevBuf<uint8_t> d_blkout;         // mfb_receive_block: the block's result record (scalars | SNR windows | symbols), one copy to the host
    DevBuf<uint8_t> d_blkout2;        // ... of flight slot 1 when a block runs as two parts on two streams (mfb_set_batch_overlap)
    BlockGraph bgraph2[2][2] = {};    // part 2's recorded graphs ([input buffer][slot]; bgraph holds part 1's, or the whole block)
    BlockScalars *d_scal = nullptr;   // = d_blkout: not owned
    int band_cap = 0;
    bool W_valid = false;
    // batches of blocks (mfb_receive_blocks_*): B consecutive blocks of ONE contiguous window of samples per launch set
    int win_blocks = 0, win_stride = 0;   // capacity in blocks and block advance (N - overlap) the windows were made for
    HostBuf<cf> h_win[2];                 // page-locked windows of win_blocks * win_stride + (N - win_stride) samples ...
    DevBuf<cf> d_win[2];                  // ... and their device copies
    Event ev_wh2d[2], ev_wfree[2];
    int bat_cap = 0;                      // blocks the batch work buffers below hold
    DevBuf<cf> d_Xb, d_xcb, d_Pb;         // spectra [B][N], matched-filter outputs [B][M][N], envelope spectra [B][N]
    DevBuf<float> d_envb, d_sumb, d_resb, d_crb;   // envelopes [B][N], doppSum [B][Dtot][M], picks [B][2], rate triples [B][3]
    DevBuf<uint8_t> d_batout;             // result records [B][rec] of the batch in flight slot 0 ...
    DevBuf<uint8_t> d_batout2;            // ... and slot 1 (the next batch's search writes its picks while this one's records are still read)
    size_t batout_cap = 0;
    // A batch in two parts on two streams (round 6).  Part 1 -- forward transforms, search, pick: the kernels that fill the chip --
    // stays on `stream`; part 2 -- matched filters at the picked shift, envelope, its spectrum, rate, centres, the integer stages,
    // the read-back: a chain of small launches that leaves most of the chip idle -- goes to `s2`, behind an event, with an
    // intermediate of its own for its transforms (d_Z2).  The next batch's part 1 then runs beside this batch's part 2.
    Event ev_p1[2];               // [slot]: part 1 of the batch in that flight has been enqueued and finished
    DevBuf<cf> d_Z2;
    size_t z2_rows = 0;
    bool use_z2 = false;          // the transforms being enqueued use d_Z2 (part 2)
    bool s2_busy = false;         // something was enqueued on s2 since the last wait for it
    bool batch_overlap = false;   // mfb_set_batch_overlap
    bool device_snr = false;      // mfb_set_device_snr
    int last_batch_blocks = 0;    // blocks of the batch begun last (mfb_get_batch_scores)
    int cu_part = 0, cu_parts = 0;        // mfb_set_cu_share (0, 0: the whole device)
    BlockGraph wgraph2[2][2][2][WG_NB + 1] = {};     // part 2's recorded graphs (wgraph holds part 1's)
    // [window][slot][carry parity][blocks of the batch]: a receive loop that takes whatever is complete (1 ... B blocks per call)
    // keeps one recorded graph per batch size it has met twice; sizes above WG_NB share entry 0 (recorded again when the size changes)
    BlockGraph wgraph[2][2][2][WG_NB + 1] = {};
    // the integer stages behind the symbol decisions on the device (stream_kernels.hpp; mfb_set_stream_stages): A12 bit lookup,
    // A13 block-overlap alignment, A14 sync search on the stream without a stash -- batches only
    bool st_on = false;
    StreamArgs st = {};           // constant part (LUTs, thresholds, templates; its pointers own nothing); records, carries filled per batch
    DevBuf<uint8_t> d_lut8;
    DevBuf<int> d_lut3;
    DevBuf<int8_t> d_sttmpl;
    DevBuf<StreamCarry> d_carry[2];   // [parity]: the previous batch's tail and bit ring / this batch's
    int carry_cur = 0;                // buffer that holds the state the next batch starts from
    HostBuf<StreamCarry> h_seed;      // page-locked staging of mfb_stream_seed
    std::vector<Event> ev[2];
    std::vector<Event> ev_pool;
    // the search with the Doppler shift on the filter side (seg_kernels.hpp, segf_body; 256-point segments): per-bin spectra
    std::vector<int> h_shifts, h_uniq;   // host copies of the shift table and of the unique-filter map
    std::vector<int> h_mult;             // how many of the M filters each unique one stands for (k_finalize counts its row that often)
    DevBuf<float> d_Qs;                  // [Dtot][L]: per-bin sum over the rows of |d_Gs|^2 (SUM_ALL searches; segf_body SUMQ), built with d_Gs
    DevBuf<cf> d_Gs;                     // [Dtot][rows][L]: rows = the unique filters, or the span basis
    int gs_rows = 0;                     // rows per bin d_Gs was built for (0: not built)
    int gs_span = -1;                    // ... and for which basis
    int gs_l = 0;                        // ... and segment length (log2)
    DevBuf<u32x4> d_Wb;                  // [Dtot][KT][2][64]: B fragments of the wrap-around outputs (wrap_kernels.hpp), built with d_Gs
    DevBuf<int> d_Wexp;                  // [Dtot]: their powers of two
    int wb_kt = 0;                       // K-steps d_Wb was built for (0: not built)
    // interference-peak clipping before the forward transform (clip_kernels.hpp, mfb_set_peak_clip; DB:670-707)
    float clip_scale = 0.f;              // 0: off
    int clip_ov = 0;                     // > 0: block b's first clip_ov samples are block b - 1's clipped tail
    bool clip_restart = false;           // the next block's overlap is taken as given
    int clip_cap[2] = {};                // blocks the flight buffers below hold, per slot
    int clip_ws_cap = 0;                 // ... and the shared workspace
    DevBuf<cf> d_clipx[2];               // [flight slot]: clipped blocks [clip_cap][N] -- what the transforms and part 2 read
    DevBuf<int> d_clipi[2], d_cliph[2];  // ... their indices [clip_cap][N] and heads [clip_cap][CLIP_HEAD]
    HostBuf<int32_t> h_cliph[2];         // page-locked copies of the heads (read back with the flight)
    DevBuf<float> d_clips;               // leaf sums of the two rounds [2][clip_ws_cap][N / 128] and thresholds [clip_ws_cap][2]
    DevBuf<int> d_clipw;                 // per-wave counts and tail flags [2][clip_ws_cap][N / 1024]
    DevBuf<ClipTail> d_ctail;            // the last clipped block's tail (stable address: captured graphs hold it)
    int ctail_cap = 0;
    // integer IQ samples in the page-locked inputs (unpack_kernels.hpp, mfb_set_sample_format): the raw bytes land in a staging
    // buffer of the input's own and k_unpack writes complex64 into the device copy everything else reads
    int fmt = MFB_SAMPLES_CF32;
    float fmt_scale = 1.f;
    DevBuf<void> d_raw[4];               // [input buffer 0 / 1, window 0 / 1]: allocated at the first copy that needs it
    size_t raw_cap[4] = {};
};

// the handle's stream and -- when a batch has put work there since the last wait -- the second stream of the batch path
static hipError_t sync_streams(mfb_ctx *c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->s2 && c->s2_busy) {
        e = hipStreamSynchronize(c->s2);
        if (e == hipSuccess) c->s2_busy = false;
    }
    return e;
}

extern "C" const char *mfb_strerror(int s) {
    switch (s) {
        case MFB_OK: return "ok";
        case MFB_ERR_ARG: return "invalid argument or shape";
        case MFB_ERR_DTYPE: return "invalid element type";
        case MFB_ERR_ALLOC: return "allocation failed";
        case MFB_ERR_HIP: return "HIP runtime error";
        case MFB_ERR_STATE: return "filters, shifts or input not set";
        case MFB_ERR_UNSUPPORTED: return "transform size not supported";
        default: return "unknown status";
    }
}
extern "C" int mfb_abi_version(void) { return 9; }

static void make_twiddles(std::vector<cf> &v, int count, double denom, double stepmul) {
    v.resize(count);
    for (int i = 0; i < count; ++i) {
        const double ang = 2.0 * M_PI * (double)i * stepmul / denom;
        v[i] = (cf){(float)cos(ang), (float)sin(ang)};
    }
}

// (cos, tan) pairs of the fused-twiddle transforms (fft_core.hpp, MFB_FFT_FUSED), appended to the W_L table: angle 2 pi u / L.
// An angle of exactly pi/2 (one lane of stage 1) becomes (2^-40, 2^40): c t = 1 exactly, and c b vanishes in the rounding of the sum.
static cf ct_pair(long u, int L) {
    const double ang = 2.0 * M_PI * (double)u / (double)L;
    double c = cos(ang);
    const double s = sin(ang);
    if (fabs(c) < 1e-9) c = 0x1p-40;
    return (cf){(float)c, (float)(s / c)};
}
static void append_fused_tables(std::vector<cf> &v, int L) {
    if (L == 256) {            // F256Regs: [16 lanes][8]
        for (int g = 0; g < 16; ++g) {
            const long u[8] = {8 * g, 4 * g, 2 * g, 2 * g + 32, g, g + 16, g + 32, g + 48};
            for (int k = 0; k < 8; ++k) v.push_back(ct_pair(u[k], L));
        }
    } else if (L == 2048) {    // F2048Regs: [64 positions][16], then W_64^p, p < 32
        for (int g = 0; g < 64; ++g) {
            v.push_back(ct_pair(16 * g, L));
            v.push_back(ct_pair(8 * g, L));
            for (int q = 0; q < 2; ++q) v.push_back(ct_pair(4 * g + 256 * q, L));
            for (int q = 0; q < 4; ++q) v.push_back(ct_pair(2 * g + 128 * q, L));
            for (int q = 0; q < 8; ++q) v.push_back(ct_pair(g + 64 * q, L));
        }
        for (int p = 0; p < 32; ++p) v.push_back(ct_pair(32 * p, L));
    }
}

static int upload_tw(DevBuf<cf> *dst, const std::vector<cf> &v) {
    HIPCHK(dst->alloc(v.size() * sizeof(cf), dev_alloc));
    HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(cf), hipMemcpyHostToDevice));
    return MFB_OK;
}

// pass-2 work split: sub-rows (n1 values) per workgroup; a power of two in [RB, N1]
static void set_rows_per_block(mfb_ctx *c, int srb) {
    const int NT = c->N2 / 16;
    const int RB = NT >= 256 ? 1 : 256 / NT;
    int p = 1;
    while (p * 2 <= srb) p *= 2;
    srb = p;
    if (srb < RB) srb = RB;
    if (srb > c->N1) srb = c->N1;
    c->srb = srb;
    c->parts = c->N1 / srb;
}

static int default_chunk(const mfb_ctx *c) {
    const size_t row_bytes = (size_t)c->N * sizeof(cf) * c->MU;
    size_t ch = ((size_t)8 << 30) / row_bytes;
    if (ch < 1) ch = 1;
    if (ch > (size_t)c->Dtot) ch = c->Dtot;
    if (ch * c->MU > 65535) ch = 65535 / c->MU;
    return (int)ch;
}

// The bookkeeping half of every grow-only reserve of a handle, for one buffer or a group that shares a capacity: free all of them,
// then allocate all of them (dev_alloc).  The capacity is 0 -- and whatever is missing empty -- until all of the group exist again.
// The policy half stays with the caller, BEFORE the call: which streams to wait for, and whether recorded graphs die (epoch,
// graph_drop).  A hipFree that fails is reported (MFB_ERR_HIP), as it always was on these paths; only teardown ignores it.
struct GrowBuf {
    Mem<DevFree> *buf;
    size_t bytes;
};
template <class Cap>
static int grow_buffers(Cap *cap, Cap want, std::initializer_list<GrowBuf> bufs) {
    *cap = 0;
    for (const GrowBuf &b : bufs) HIPCHK(b.buf->reset());
    for (const GrowBuf &b : bufs) HIPCHK(b.buf->alloc(b.bytes, dev_alloc));
    *cap = want;
    return MFB_OK;
}

// Intermediate of the two-pass transforms.  The segment path needs one row only (the plain forward
// transforms of A3 / A10 still run two-pass); the two-pass search needs chunk * MU rows.
static size_t z_rows_needed(const mfb_ctx *c) {
    if (!c->have_filters || c->path == MFB_PATH_SEGMENT) return 1;
    if (c->search_mode == MFB_SEARCH_ENERGY) return (size_t)c->M;   // the demodulation stage only
    const size_t rows = (size_t)c->chunk * c->MU;   // the search stores only the unique filter rows
    return rows > (size_t)c->M ? rows : (size_t)c->M;
}
static int alloc_Z(mfb_ctx *c) {
    const size_t need = z_rows_needed(c);
    if (c->d_Z && c->z_rows >= need) return MFB_OK;
    if (c->d_Z) HIPCHK(sync_streams(c));
    return grow_buffers(&c->z_rows, need, {{&c->d_Z, need * c->N * sizeof(cf)}});
}

static int reserve_partials(mfb_ctx *c, size_t floats) {
    if (c->part_cap >= floats) return MFB_OK;
    if (c->d_part) {
        HIPCHK(sync_streams(c));
        ++c->epoch;          // recorded block graphs hold the old address
    }
    return grow_buffers(&c->part_cap, floats, {{&c->d_part, floats * sizeof(float)}});
}

// Device-side result record of a block: [BlockScalars, 256 B][bands 2 x bcap complex64][sym][cen][mag] (nthreads each),
// contiguous so that ONE copy brings it to the host.
// The layout itself is stated in record_layout.hpp; everything below asks rec_layout.
#define BLK_HEAD 256
static_assert(sizeof(BlockScalars) <= BLK_HEAD && sizeof(cf) == 2 * sizeof(float), "record_layout.hpp counts on both");
static RecordLayout rec_layout(int bcap, int nthreads, bool stages = false) {
    static const RecordConsts k = {BLK_HEAD, STREAM_POST_MAX, STREAM_END_MAX, STREAM_MAX_TMPL, STREAM_MAX_HITS, STREAM_EDGE_CANDS, sizeof(StreamEdge)};
    return record_layout(k, bcap, nthreads, stages);
}
static int blkout_reserve(mfb_ctx *c, int bcap) {
    if (c->d_blkout && bcap <= c->band_cap) return MFB_OK;
    HIPCHK(sync_streams(c));
    if (c->d_blkout) ++c->epoch;       // captured block graphs hold the old record's address (and d_scal): none of them may replay
    c->band_cap = 0;
    const size_t bytes = rec_layout(bcap, c->cap).bytes;
    HIPCHK(c->d_blkout.alloc(bytes, dev_alloc));
    HIPCHK(c->d_blkout2.alloc(bytes, dev_alloc));        // flight slot 1 (two streams: mfb_set_batch_overlap)
    c->band_cap = bcap;
    c->d_scal = (BlockScalars *)c->d_blkout.get();
    return MFB_OK;
}

// ---- per-device kernel attributes ------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): it is set for every
// instantiation that can need more than 48 KiB whenever a handle is created, on that handle's device.
template <int L1>
static int attr_p1() {
    if (P1Cfg<L1>::lds_bytes > 48 * 1024) {
        const int b = (int)P1Cfg<L1>::lds_bytes;
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_BANK>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_FWDC>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass1<L1, KIND_FWDR>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
    }
    return MFB_OK;
}
template <int L2>
static int attr_p2() {
    if (P2Cfg<L2>::lds_bytes > 48 * 1024) {
        const int b = (int)P2Cfg<L2>::lds_bytes;
        HIPCHK(hipFuncSetAttribute((const void *)k_pass2<L2, MODE_REDUCE>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        HIPCHK(hipFuncSetAttribute((const void *)k_pass2<L2, MODE_STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
    }
    return MFB_OK;
}
// ---- the search's kernel instantiations, enumerated ONCE per family ----------------------------------------------------------------
// visit_*(f) calls f(tag) for every instantiation of the family until a call returns something other than VISIT_NEXT, and returns
// that.  Setting the attributes visits all of a family; a launch visits until (segment length, mode or variant, pv) matches.  The
// ranges are seg_ppl, segf_has_sumq and segf_has_presum themselves, and nothing else is instantiated: no launch reaches a kernel whose
// attribute was never set.  PV: valid register slots of a complete segment (half ... all) for the branch-free form, -1 = masked.
constexpr int VISIT_NEXT = -1;
template <int SEGL_, int MODE_, int PV_>
struct SegInst {       // k_seg<L, MODE, PV> | k_segf<L, PV, SUMQ = MODE>
    static constexpr int SEGL = SEGL_, L = 1 << SEGL_, MODE = MODE_, PV = PV_;
};
template <int SEGL, class F, int... I>
static int visit_seg_l(F &f, std::integer_sequence<int, I...>) {
    int rc = f(SegInst<SEGL, SEG_STORE, -1>{});
    if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, SEG_REDUCE, -1>{});
    (void)((rc == VISIT_NEXT && (rc = f(SegInst<SEGL, SEG_REDUCE, seg_ppl(1 << SEGL) / 2 + I>{})) == VISIT_NEXT) && ...);
    return rc;
}
using SegLens = std::integer_sequence<int, 8, 9, 10, 11, 12, SEG_LOG2L_MAX>;
template <class F, int... SEGL>
static int visit_seg(F f, std::integer_sequence<int, SEGL...>) {
    int rc = VISIT_NEXT;
    (void)(((rc = visit_seg_l<SEGL>(f, SegSlots<(1 << SEGL)>{})) == VISIT_NEXT) && ...);
    return rc;
}
template <int SEGL, class F, int... I>
static int visit_segf_l(F &f, std::integer_sequence<int, I...>) {
    int rc = VISIT_NEXT;
    auto variants = [&](auto pv) {
        constexpr int L = 1 << SEGL, PV = decltype(pv)::value;
        rc = f(SegInst<SEGL, 0, PV>{});
        if constexpr (segf_has_sumq<L, PV>())
            if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, 1, PV>{});
        if constexpr (segf_has_presum<L, PV>())
            if (rc == VISIT_NEXT) rc = f(SegInst<SEGL, 2, PV>{});
        return rc == VISIT_NEXT;
    };
    (void)(variants(std::integral_constant<int, seg_ppl(1 << SEGL) / 2 + I>{}) && ...);
    return rc;
}
template <class F>
static int visit_segf(F f) {
    const int rc = visit_segf_l<8>(f, SegSlots<256>{});
    return rc != VISIT_NEXT ? rc : visit_segf_l<11>(f, SegSlots<2048>{});
}
#define MFB_MAX_LDS(K_, B_) HIPCHK(hipFuncSetAttribute((const void *)K_, hipFuncAttributeMaxDynamicSharedMemorySize, B_))
static int set_kernel_attributes(const mfb_ctx *c) {
    int rc = MFB_OK;
    switch (c->l1) {
        case 5: rc = attr_p1<32>(); break;
        case 6: rc = attr_p1<64>(); break;
        case 7: rc = attr_p1<128>(); break;
        case 8: rc = attr_p1<256>(); break;
        case 9: rc = attr_p1<512>(); break;
    }
    if (rc) return rc;
    switch (c->l2) {
        case 13: rc = attr_p2<8192>(); break;
        default: break;   // <= 4096 points: 35 KiB
    }
    if (rc) return rc;
    rc = visit_seg([](auto k) -> int {
        using K = decltype(k);
        MFB_MAX_LDS((k_seg<K::L, K::MODE, K::PV>), seg_lds_bytes(K::SEGL, SEG_REDUCE, seg_mpb_cap(K::SEGL)));
        return VISIT_NEXT;
    }, SegLens{});
    if (rc == VISIT_NEXT)
        rc = visit_segf([](auto k) -> int {
            using K = decltype(k);
            MFB_MAX_LDS((k_segf<K::L, K::PV, K::MODE>), segf_lds_bytes<K::L>(segf_rows_cap(K::L)));
            return VISIT_NEXT;
        });
    if (rc != VISIT_NEXT) return rc;
    MFB_MAX_LDS((k_segw<SEGW_PV, SEGW_KT>), segw_lds_bytes());
    return MFB_OK;
}
#undef MFB_MAX_LDS

static int create_impl(mfb_ctx *c) {
    HIPCHK(hipStreamCreateWithFlags(out(c->own_stream), hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIPCHK(hipEventCreate(out(c->t0)));
    HIPCHK(hipEventCreate(out(c->t1)));
    int rc = set_kernel_attributes(c);
    if (rc) return rc;
    const int M = c->M;
    const size_t nb = (size_t)c->N * sizeof(cf);
    HIPCHK(c->h_in.alloc(nb, hip_host_malloc));
    memset(c->h_in, 0, nb);
    // three arrays of at most N/2 symbol decisions, the block scalars and the two SNR windows of mfb_receive_block
    c->back_cap = (size_t)3 * (c->N / 2) * sizeof(int) + ((size_t)256 << 10);
    if (c->back_cap < ((size_t)64 << 10)) c->back_cap = (size_t)64 << 10;
    HIPCHK(c->h_back.alloc(c->back_cap, hip_host_malloc));
    HIPCHK(c->h_pick.alloc(4 * sizeof(uint32_t), hip_host_malloc_coherent));
    memset(c->h_pick, 0, 4 * sizeof(uint32_t));          // pick 0 is never asked for
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_pick_dev, c->h_pick, 0));
    HIPCHK(c->d_x.alloc(nb, dev_alloc));
    HIPCHK(c->d_X.alloc(nb, dev_alloc));
    HIPCHK(c->d_masks.alloc(nb * M, dev_alloc));
    HIPCHK(c->d_xc.alloc(nb * M, dev_alloc));
    HIPCHK(c->d_P.alloc(nb, dev_alloc));
    HIPCHK(c->d_env.alloc((size_t)c->N * sizeof(float), dev_alloc));
    HIPCHK(c->d_shifts.alloc((size_t)c->Dtot * sizeof(int), dev_alloc));
    if ((rc = reserve_partials(c, (size_t)c->Dtot * M * c->N1))) return rc;
    HIPCHK(c->d_sum.alloc((size_t)c->Dtot * M * sizeof(float), dev_alloc));
    HIPCHK(hipMemset(c->d_sum, 0, (size_t)c->Dtot * M * sizeof(float)));
    HIPCHK(c->d_res.alloc(2 * sizeof(float), dev_alloc));
    HIPCHK(c->d_uniq.alloc((size_t)M * sizeof(int), dev_alloc));
    HIPCHK(c->d_rep.alloc((size_t)M * sizeof(int), dev_alloc));
    HIPCHK(c->d_cr.alloc(3 * sizeof(float), dev_alloc));
    c->cap = c->N / 2;  // symbols never shorter than 2 samples
    HIPCHK(c->d_sym.alloc((size_t)c->cap * sizeof(int), dev_alloc));
    HIPCHK(c->d_cen.alloc((size_t)c->cap * sizeof(int), dev_alloc));
    HIPCHK(c->d_mag.alloc((size_t)c->cap * sizeof(float), dev_alloc));
    // one row for the plain forward transforms; the search's share is sized when the filters arrive
    if ((rc = alloc_Z(c))) return rc;
    // block path (mfb_receive_block*): everything it needs exists before the first block -- page-locking memory and creating
    // events inside a stream of blocks costs milliseconds
    if ((rc = blkout_reserve(c, 1024))) return rc;
    for (int i = 0; i < 2; ++i) {
        // scalars + three arrays of the symbols a rate window of +-10 % around 4 samples per symbol admits + the two windows
        c->blk_cap[i] = rec_layout(c->band_cap, c->N / 3).bytes;
        HIPCHK(c->h_blk[i].alloc(c->blk_cap[i], hip_host_malloc));
        HIPCHK(hipEventCreateWithFlags(out(c->ev_blk[i]), hipEventDisableTiming));
    }

    std::vector<cf> t;
    make_twiddles(t, c->N1, (double)c->N1, 1.0);
    if ((rc = upload_tw(&c->d_tw1, t))) return rc;
    make_twiddles(t, c->N2, (double)c->N2, 1.0);
    if ((rc = upload_tw(&c->d_tw2, t))) return rc;
    make_twiddles(t, 1 << c->lo, (double)c->N, 1.0);
    if ((rc = upload_tw(&c->d_twLo, t))) return rc;
    make_twiddles(t, c->N >> c->lo, (double)c->N, (double)(1 << c->lo));
    if ((rc = upload_tw(&c->d_twHi, t))) return rc;
    c->d_in = c->d_x;
    return MFB_OK;
}

struct CtxDestroy {
    void operator()(mfb_ctx *c) const { (void)mfb_destroy(c); }
};
static int create_body(mfb_ctx **out, int device, int log2N, int num_dopplers, int doppler_offset, int M,
                       int window_width, int sum_all_masks, int code_search_mask_offset) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    if (num_dopplers < 1 || doppler_offset < 0 || M < 1 || M > 64 || window_width < 1 || (window_width & 1) == 0 ||
        code_search_mask_offset < 0 || 2 * code_search_mask_offset >= M)
        return MFB_ERR_ARG;
    if (log2N < 10 || log2N > 22) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));

    // any failure below -- a status or an exception -- frees what was allocated so far (mfb_destroy tolerates partial handles):
    // the counterpart of the reference's context teardown, demodulator_base.py:517-530
    std::unique_ptr<mfb_ctx, CtxDestroy> c(new mfb_ctx());
    c->device = device;
    c->num_cus = ncu > 0 ? ncu : 256;
    c->log2N = log2N;
    c->N = 1 << log2N;
    // N = N1 * N2: columns of at most 256 points, rows of at most 8192 (2^22 = 512 x 8192: a 16384-point row would
    // need 1024 threads at 128 VGPRs and spilled > 100 registers)
    c->l1 = log2N / 2 < 8 ? log2N / 2 : 8;
    if (log2N - c->l1 > 13) c->l1 = log2N - 13;
    c->l2 = log2N - c->l1;
    c->N1 = 1 << c->l1;
    c->N2 = 1 << c->l2;
    c->lo = (log2N + 1) / 2;
    c->D = num_dopplers;
    c->Doff = doppler_offset;
    c->Dtot = num_dopplers + doppler_offset;
    c->M = M;
    c->W = window_width;
    c->sum_all = sum_all_masks ? 1 : 0;
    c->cs_off = code_search_mask_offset;
    // Two-pass search, Doppler bins per launch: as many as an 8 GiB intermediate holds.  Measured on
    // MI355X (C2: D=256, M=8, N=2^20): long persistent loops amortise the per-workgroup twiddle setup
    // and keep each XCD's L2 serving the filter tile to many Doppler streams, so big chunks win (chunk
    // 16: 9.8 ms, 64: 6.65 ms, 128: 6.55 ms per block) -- but a 16 GiB intermediate (chunk 256) costs
    // 0.4 ms more than two 8 GiB launches.  Keeping the intermediate inside the 256 MiB Infinity
    // Cache (chunk 1-2) does not pay: the cache streams no faster than HBM (tools/ubench/mall.hip).
    c->MU = M;
    c->chunk_auto = true;
    c->chunk = default_chunk(c.get());
    c->mpb = M < 8 ? M : 8;
    c->jsplit = 32;
    set_rows_per_block(c.get(), 64);
    c->path_req = MFB_PATH_AUTO;
    c->path = MFB_PATH_TWOPASS;
    if ((rc = create_impl(c.get()))) return rc;
    *out = c.release();
    return MFB_OK;
}
extern "C" int mfb_create(mfb_ctx **out, int device, int log2N, int num_dopplers, int doppler_offset, int M,
                          int window_width, int sum_all_masks, int code_search_mask_offset) {
    return guarded([&] { return create_body(out, device, log2N, num_dopplers, doppler_offset, M, window_width, sum_all_masks, code_search_mask_offset); });
}

static void graph_drop(BlockGraph &g);
// every recorded graph of the handle, or (slot >= 0) those of one flight slot
template <class F>
static void for_each_graph(mfb_ctx *c, int slot, F &&f) {
    for (int in = 0; in < 2; ++in)
        for (int s = 0; s < 2; ++s) {
            if (slot >= 0 && s != slot) continue;
            f(c->bgraph[in][s]);
            f(c->bgraph2[in][s]);
            for (int par = 0; par < 2; ++par)
                for (int nb = 0; nb <= WG_NB; ++nb) {
                    f(c->wgraph[in][s][par][nb]);
                    f(c->wgraph2[in][s][par][nb]);
                }
        }
}
extern "C" int mfb_destroy(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->s2) (void)hipStreamSynchronize(c->s2);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->in_stream) (void)hipStreamSynchronize(c->in_stream);
    for_each_graph(c, -1, graph_drop);
    delete c;       // ~mfb_ctx: every buffer and event, then the streams (see the struct)
    return MFB_OK;
}

extern "C" int mfb_set_stream(mfb_ctx *c, void *s) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    ++c->epoch;
    return MFB_OK;
}

// A share of the device's compute units for this handle's launches (include/mfbank.h): the handle's own stream is replaced by one
// created with a CU mask -- compute unit i belongs to part i % parts.
extern "C" int mfb_set_cu_share(mfb_ctx *c, int part, int parts) {
    if (!c || parts < 1 || parts > 16 || part < 0 || part >= parts) return MFB_ERR_ARG;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    Stream fresh;
    if (parts == 1) {
        HIPCHK(hipStreamCreateWithFlags(out(fresh), hipStreamNonBlocking));
    } else {
        const int words = (c->num_cus + 31) / 32;
        std::vector<uint32_t> mask((size_t)words, 0u);
        int mine = 0;
        for (int i = 0; i < c->num_cus; ++i)
            if (i % parts == part) {
                mask[(size_t)i / 32] |= 1u << (i % 32);
                ++mine;
            }
        if (!mine) return MFB_ERR_ARG;
        HIPCHK(hipExtStreamCreateWithCUMask(out(fresh), (uint32_t)words, mask.data()));
    }
    const bool was_own = c->stream == c->own_stream;
    std::swap(c->own_stream, fresh);
    if (was_own) c->stream = c->own_stream;
    c->cu_part = part;
    c->cu_parts = parts;
    ++c->epoch;
    HIPCHK(fresh.reset());        // (the old one; the handle is whole whatever this says)
    return MFB_OK;
}

extern "C" int mfb_set_tuning(mfb_ctx *c, int chunk, int mpb, int rows_per_block, int jsplit) {
    if (!c || chunk < 0 || mpb < 0 || rows_per_block < 0 || jsplit < 0) return MFB_ERR_ARG;
    ++c->epoch;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    if (rows_per_block > 0) set_rows_per_block(c, rows_per_block);
    if (jsplit > 0) c->jsplit = jsplit;
    if (chunk > 0) {
        c->chunk = chunk > c->Dtot ? c->Dtot : chunk;
        c->chunk_auto = false;
    }
    if (c->chunk * c->MU > 65535) c->chunk = 65535 / c->MU;  // grid.y limit of pass 2
    if (mpb > 0) c->mpb = mpb > c->M ? c->M : mpb;
    if (!c->have_filters) return MFB_OK;   // the intermediate is sized when the filters arrive
    return alloc_Z(c);
}
extern "C" int mfb_get_tuning(mfb_ctx *c, int *chunk, int *mpb, int *rows_per_block, int *jsplit) {
    if (!c) return MFB_ERR_ARG;
    if (chunk) *chunk = c->chunk;
    if (mpb) *mpb = c->mpb;
    if (rows_per_block) *rows_per_block = c->srb;
    if (jsplit) *jsplit = c->jsplit;
    return MFB_OK;
}

extern "C" int mfb_get_info(mfb_ctx *c, int *N1, int *N2, int *unique_filters) {
    if (!c) return MFB_ERR_ARG;
    if (N1) *N1 = c->N1;
    if (N2) *N2 = c->N2;
    if (unique_filters) *unique_filters = c->MU;
    return MFB_OK;
}

// ---- search path ---------------------------------------------------------------------------------
// What the planner (search_plan.hpp) is asked for this handle: the only bridge between the two.
static SearchInputs search_inputs(const mfb_ctx *c) {
    SearchInputs in = search_env();       // (the switches)
    in.N = c->N, in.Dtot = c->Dtot, in.M = c->M, in.MU = c->MU, in.MB = c->MB;
    in.sum_all = c->sum_all;
    in.uniform_mult = std::all_of(c->h_mult.begin(), c->h_mult.end(), [&](int m) { return m == c->h_mult[0]; });
    in.T = c->bank ? c->bank->T : 0;
    in.basis_req = c->basis_req, in.path_req = c->path_req, in.segl_req = c->segl_req, in.seg_wpc = c->seg_wpc, in.seg_mpb = c->seg_mpb;
    in.num_cus = c->num_cus;
    in.shifts_known = (int)c->h_shifts.size() == c->Dtot;
    return in;
}
static Segments segments(const mfb_ctx *c) { return Segments{c->path, c->segl, c->V, c->T, c->Q, c->basis, true}; }   // (those in force)

static int fsm_prepare_eager(mfb_ctx *c);
// settle path and segment length from the request and the analysed bank; (re)build G and W_L
static int resolve_path(mfb_ctx *c) {
    ++c->epoch;               // whatever changes here changes the launches of a block
    if (!c->have_filters || !c->bank) return MFB_OK;
    const Segments sg = resolve_segments(search_inputs(c));
    if (!sg.ok) return MFB_ERR_UNSUPPORTED;
    const int l = sg.segl;
    HIPCHK(sync_streams(c));
    if (!l) {
        c->path = MFB_PATH_TWOPASS;
        c->segl = 0;
        c->basis = MFB_BASIS_FILTERS;
    } else {
        const int L = 1 << l;
        if (c->segl != l || !c->d_G) {
            std::vector<float> G;
            taps::segment_spectra(*c->bank, L, sg.T, &G, seg_ppl(L));
            HIPCHK(c->d_G.alloc(G.size() * sizeof(float), dev_alloc));
            HIPCHK(hipMemcpy(c->d_G, G.data(), G.size() * sizeof(float), hipMemcpyHostToDevice));
            if (c->twL_len != L) {
                c->twL_len = 0;
                std::vector<cf> t;
                make_twiddles(t, L, (double)L, 1.0);
                append_fused_tables(t, L);
                int rc = upload_tw(&c->d_twL, t);
                if (rc) return rc;
                c->twL_len = L;
            }
        }
        // opt-in span basis of the SUM_ALL search: its rank is found here, and the basis settled with it
        if (c->basis_req == MFB_BASIS_SPAN && c->sum_all) {
            if (c->gb_l != l || !c->d_Gb) {
                taps::Bank sb;
                c->MB = taps::span_basis(*c->bank, &sb);
                std::vector<float> G;
                if (c->MB > 0) taps::segment_spectra(sb, L, sg.T, &G, seg_ppl(L));
                HIPCHK(c->d_Gb.reset());
                c->gb_l = 0;
                if (c->MB > 0) {
                    HIPCHK(c->d_Gb.alloc(G.size() * sizeof(float), dev_alloc));
                    HIPCHK(hipMemcpy(c->d_Gb, G.data(), G.size() * sizeof(float), hipMemcpyHostToDevice));
                    c->gb_l = l;
                }
            }
        }
        c->path = MFB_PATH_SEGMENT;
        c->segl = l;
        c->V = sg.V;
        c->T = sg.T;                  // taps the segments are laid out for (>= the bank's T)
        c->win_start = c->bank->start;
        c->Q = sg.Q;
        c->basis = resolve_segments(search_inputs(c)).basis;
    }
    if (c->path == MFB_PATH_TWOPASS) {
        if (c->chunk_auto) c->chunk = default_chunk(c);
        if (c->chunk * c->MU > 65535) c->chunk = 65535 / c->MU;
        int rc = reserve_partials(c, (size_t)c->Dtot * c->M * c->N1);
        if (rc) return rc;
    } else if (c->d_Z && c->z_rows > 1) {   // give the big intermediate back
        c->z_rows = 0;
        HIPCHK(c->d_Z.reset());
    }
    int rc = alloc_Z(c);
    if (rc) return rc;
    return fsm_prepare_eager(c);
}

static int set_search_path_body(mfb_ctx *c, int path, int log2L, int wg_per_cu, int filters_per_pass) {
    if (!c || path < 0 || path > MFB_PATH_SEGMENT || log2L < 0 || wg_per_cu < 0 || wg_per_cu > 64 || filters_per_pass < 0 ||
        filters_per_pass > SEG_MPB_MAX)
        return MFB_ERR_ARG;
    if (log2L && (log2L < 8 || log2L > SEG_LOG2L_MAX)) return MFB_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(c->device));
    const int old_path = c->path_req, old_l = c->segl_req, old_wpc = c->seg_wpc, old_mpb = c->seg_mpb;
    c->path_req = path;
    c->segl_req = log2L;
    c->seg_wpc = wg_per_cu;
    c->seg_mpb = filters_per_pass;
    const int rc = resolve_path(c);
    if (rc) {           // keep the previous, working configuration
        c->path_req = old_path;
        c->segl_req = old_l;
        c->seg_wpc = old_wpc;
        c->seg_mpb = old_mpb;
        (void)resolve_path(c);
    }
    return rc;
}
extern "C" int mfb_set_search_path(mfb_ctx *c, int path, int log2L, int wg_per_cu, int filters_per_pass) {
    return guarded([&] { return set_search_path_body(c, path, log2L, wg_per_cu, filters_per_pass); });
}

static int set_search_basis_body(mfb_ctx *c, int basis) {
    if (!c || (basis != MFB_BASIS_FILTERS && basis != MFB_BASIS_SPAN)) return MFB_ERR_ARG;
    if (basis == MFB_BASIS_SPAN && !c->sum_all) return MFB_ERR_STATE;   // per-filter sums need every filter
    HIPCHK(hipSetDevice(c->device));
    c->basis_req = basis;
    return resolve_path(c);
}
extern "C" int mfb_set_search_basis(mfb_ctx *c, int basis) {
    return guarded([&] { return set_search_basis_body(c, basis); });
}
static int set_search_mode_body(mfb_ctx *c, int mode) {
    if (!c || (mode != MFB_SEARCH_TRANSFORMS && mode != MFB_SEARCH_ENERGY)) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    c->search_mode = mode;
    return resolve_path(c);      // the two-pass intermediate is sized for what the search needs
}
extern "C" int mfb_set_search_mode(mfb_ctx *c, int mode) {
    return guarded([&] { return set_search_mode_body(c, mode); });
}
extern "C" int mfb_get_search_mode(mfb_ctx *c, int *mode) {
    if (!c || !mode) return MFB_ERR_ARG;
    *mode = c->search_mode;
    return MFB_OK;
}
extern "C" int mfb_get_search_basis(mfb_ctx *c, int *basis, int *transformed_filters) {
    if (!c) return MFB_ERR_ARG;
    if (basis) *basis = c->basis;
    if (transformed_filters) *transformed_filters = (c->path == MFB_PATH_SEGMENT && c->basis == MFB_BASIS_SPAN) ? c->MB : c->MU;
    return MFB_OK;
}
static int analyze_rank_body(const float *masks, int M, int N, int *rank) {
    if (!masks || !rank || M < 1 || N < 2 || (N & (N - 1))) return MFB_ERR_ARG;
    taps::Bank b, sb;
    taps::analyse(masks, M, N, &b);
    if (b.T > taps::ROW_TAPS_MAX) {
        *rank = M;          // no short support: not analysed
        return MFB_OK;
    }
    *rank = taps::span_basis(b, &sb);
    return MFB_OK;
}
extern "C" int mfb_analyze_rank(const float *masks, int M, int N, int *rank) {
    return guarded([&] { return analyze_rank_body(masks, M, N, rank); });
}

extern "C" int mfb_get_search_path(mfb_ctx *c, int *path, int *log2L, int *taps_out, int *valid_per_segment, int *segments) {
    if (!c) return MFB_ERR_ARG;
    if (path) *path = c->path;
    if (log2L) *log2L = c->segl;
    if (taps_out) *taps_out = c->bank ? c->bank->T : 0;
    if (valid_per_segment) *valid_per_segment = c->path == MFB_PATH_SEGMENT ? c->V : 0;
    if (segments) *segments = c->path == MFB_PATH_SEGMENT ? c->Q : 0;
    return MFB_OK;
}

static int analyze_filters_body(const float *masks, int M, int N, int *support_start, int *support_len) {
    if (!masks || M < 1 || N < 2 || (N & (N - 1))) return MFB_ERR_ARG;
    taps::Bank b;
    taps::analyse(masks, M, N, &b);
    if (support_start) *support_start = b.start;
    if (support_len) *support_len = b.T;
    return MFB_OK;
}
extern "C" int mfb_analyze_filters(const float *masks, int M, int N, int *support_start, int *support_len) {
    return guarded([&] { return analyze_filters_body(masks, M, N, support_start, support_len); });
}

static int set_filters_body(mfb_ctx *c, const float *masks, int M, int N) {
    if (!c || !masks) return MFB_ERR_ARG;
    if (M != c->M || N != c->N) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_masks, masks, (size_t)M * N * sizeof(cf), hipMemcpyHostToDevice, c->stream));
    // Filters that are exact copies or exact negatives of an earlier one (the BPSK bank: pattern p
    // and its complement) give bit-identical |.|^2; the Doppler search transforms each such class once.
    std::vector<int> uniq, rep(M);
    for (int m = 0; m < M; ++m) {
        const float *rm = masks + (size_t)m * 2 * N;
        int found = -1;
        for (size_t u = 0; u < uniq.size() && found < 0; ++u) {
            const float *ru = masks + (size_t)uniq[u] * 2 * N;
            bool same = true, neg = true;
            for (size_t i = 0; i < (size_t)2 * N && (same || neg); ++i) {
                same = same && (rm[i] == ru[i]);
                neg = neg && (rm[i] == -ru[i]);
            }
            if (same || neg) found = (int)u;
        }
        if (found < 0) {
            found = (int)uniq.size();
            uniq.push_back(m);
        }
        rep[m] = found;
    }
    c->MU = (int)uniq.size();
    c->h_uniq = uniq;
    c->h_mult.assign(uniq.size(), 0);
    for (int m = 0; m < M; ++m) ++c->h_mult[(size_t)rep[m]];
    c->gs_rows = 0;
    HIPCHK(hipMemcpyAsync(c->d_uniq, uniq.data(), uniq.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_rep, rep.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // impulse-response window and taps of every filter (double precision, host threads)
    if (!c->bank) c->bank.reset(new taps::Bank());
    taps::analyse(masks, M, N, c->bank.get());
    HIPCHK(sync_streams(c));
    c->have_filters = true;
    c->have_xc = false;
    c->W_valid = false;
    ++c->epoch;
    c->segl = 0;    // force G to be rebuilt for the new bank
    c->gb_l = 0;
    int rc = resolve_path(c);
    if (rc == MFB_ERR_UNSUPPORTED) {   // a segment path was demanded but this bank has no short support
        c->path_req = MFB_PATH_AUTO;
        rc = resolve_path(c);
    }
    if (rc) c->have_filters = false;
    return rc;
}
extern "C" int mfb_set_filters(mfb_ctx *c, const float *masks, int M, int N) {
    bool thrown = true;
    const int rc = guarded([&] {
        const int r = set_filters_body(c, masks, M, N);
        thrown = false;
        return r;
    });
    if (thrown && c) c->have_filters = false;      // half a bank: the next mfb_set_filters starts over
    return rc;
}

static int set_shifts_body(mfb_ctx *c, const int32_t *shifts, int count) {
    if (!c || !shifts || count != c->Dtot) return MFB_ERR_ARG;
    for (int i = 0; i < count; ++i)
        if (shifts[i] < 0 || shifts[i] >= c->N) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_shifts, shifts, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_streams(c));
    // (a caller that sets the same table again -- a tracking loop, a re-attached shard -- keeps the per-bin spectra: 35 ms at C2)
    const bool same = (int)c->h_shifts.size() == count && std::equal(shifts, shifts + count, c->h_shifts.begin());
    c->h_shifts.assign(shifts, shifts + count);
    if (!same) c->gs_rows = 0;    // the per-bin spectra belong to the old table
    c->have_shifts = true;
    ++c->epoch;
    return fsm_prepare_eager(c);
}
extern "C" int mfb_set_shifts(mfb_ctx *c, const int32_t *shifts, int count) {
    return guarded([&] { return set_shifts_body(c, shifts, count); });
}

extern "C" int mfb_input_buffer(mfb_ctx *c, float **p) {
    if (!c || !p) return MFB_ERR_ARG;
    if (c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the buffer holds integers: mfb_input_buffer_raw
    *p = (float *)c->h_in.get();
    return MFB_OK;
}

// ---- launch helpers ------------------------------------------------------------------------------
static int fin_threads(int rows) { return 64 * (rows < 1 ? 1 : (rows > 16 ? 16 : rows)); }   // k_finalize: one wave per row
static Event get_event(mfb_ctx *c) {
    Event e;
    if (!c->ev_pool.empty()) {
        e = std::move(c->ev_pool.back());
        c->ev_pool.pop_back();
    } else {
        (void)hipEventCreate(out(e));      // (empty when that fails)
    }
    return e;
}
// Profiling marks come in pairs (begin, end); a mark that cannot be created or recorded switches profiling off and drops
// the marks taken so far, so that mfb_profile_read never pairs events of different launches.
static void prof_mark(mfb_ctx *c, int which) {
    if (!c->prof) return;
    Event e = get_event(c);
    if (!e || hipEventRecord(e, c->stream) != hipSuccess) {
        fprintf(stderr, "mfbank: profiling event unavailable, profiling disabled\n");
        if (e) c->ev_pool.push_back(std::move(e));
        for (auto &v : c->ev) {
            for (auto &q : v) c->ev_pool.push_back(std::move(q));
            v.clear();
        }
        c->prof = false;
        return;
    }
    c->ev[which].push_back(std::move(e));
}

template <int L1, int KIND>
static int launch_p1_t(mfb_ctx *c, const P1Args &a, dim3 grid) {
    const size_t lds = P1Cfg<L1>::lds_bytes;   // > 48 KiB cases: set_kernel_attributes (per device)
    hipLaunchKernelGGL((k_pass1<L1, KIND>), grid, dim3((L1 / 16) * TILE), lds, c->stream, a);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}
template <int KIND>
static int launch_p1(mfb_ctx *c, const P1Args &a, dim3 grid) {
    switch (c->l1) {
        case 5: return launch_p1_t<32, KIND>(c, a, grid);
        case 6: return launch_p1_t<64, KIND>(c, a, grid);
        case 7: return launch_p1_t<128, KIND>(c, a, grid);
        case 8: return launch_p1_t<256, KIND>(c, a, grid);
        case 9: return launch_p1_t<512, KIND>(c, a, grid);
    }
    return MFB_ERR_UNSUPPORTED;
}

template <int L2, int MODE>
static int launch_p2_t(mfb_ctx *c, const P2Args &a, dim3 grid) {
    constexpr int NT = L2 / 16;
    constexpr int RB = P2Cfg<L2>::RB;
    const size_t lds = P2Cfg<L2>::lds_bytes;   // > 48 KiB cases: set_kernel_attributes (per device)
    hipLaunchKernelGGL((k_pass2<L2, MODE>), grid, dim3(NT * RB), lds, c->stream, a);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}
template <int MODE>
static int launch_p2(mfb_ctx *c, const P2Args &a, dim3 grid) {
    switch (c->l2) {
        case 5: return launch_p2_t<32, MODE>(c, a, grid);
        case 6: return launch_p2_t<64, MODE>(c, a, grid);
        case 7: return launch_p2_t<128, MODE>(c, a, grid);
        case 8: return launch_p2_t<256, MODE>(c, a, grid);
        case 9: return launch_p2_t<512, MODE>(c, a, grid);
        case 10: return launch_p2_t<1024, MODE>(c, a, grid);
        case 11: return launch_p2_t<2048, MODE>(c, a, grid);
        case 12: return launch_p2_t<4096, MODE>(c, a, grid);
        case 13: return launch_p2_t<8192, MODE>(c, a, grid);
    }
    return MFB_ERR_UNSUPPORTED;
}

static P1Args p1_base(mfb_ctx *c) {
    P1Args a;
    memset(&a, 0, sizeof(a));
    a.masks = c->d_masks;
    a.Z = c->use_z2 ? c->d_Z2 : c->d_Z;
    a.tw1 = c->d_tw1;
    a.twLo = c->d_twLo;
    a.twHi = c->d_twHi;
    a.N = c->N;
    a.N2 = c->N2;
    a.lo = c->lo;
    a.M = c->M;
    a.mpb = c->mpb;
    return a;
}
// rows per workgroup for the STORE transforms (1 or M rows only): small, so the launch fills the chip
static void p2_store_split(mfb_ctx *c, P2Args &b, int rows) {
    const int NT = c->N2 / 16;
    const int RB = NT >= 256 ? 1 : 256 / NT;
    int srb = rows >= 4 ? 2 : 1;
    if (srb < RB) srb = RB;
    if (srb > c->N1) srb = c->N1;
    b.srb = srb;
    b.parts = c->N1 / srb;
}

static P2Args p2_base(mfb_ctx *c) {
    P2Args a;
    memset(&a, 0, sizeof(a));
    a.Z = c->use_z2 ? c->d_Z2 : c->d_Z;
    a.tw2 = c->d_tw2;
    a.N = c->N;
    a.N1 = c->N1;
    a.N2 = c->N2;
    a.srb = c->srb;
    a.parts = c->parts;
    a.scale = 1.0f / 262144.0f;
    return a;
}

static int launch_transpose(mfb_ctx *c, cf *dst, int rows, int conj) {
    dim3 grid((c->N2 + 31) / 32, (c->N1 + 31) / 32, rows);
    hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, c->stream, (const cf *)(c->use_z2 ? c->d_Z2 : c->d_Z), dst, c->N1, c->N2, conj);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}

// forward FFT of `rows` rows (a batch of blocks: row r reads its input in_stride elements behind row r - 1 and goes to
// dst + r * N): complex (src_c) or real (src_r) input -> dst natural order.  d_Z must hold `rows` rows.
static int forward_fft(mfb_ctx *c, const cf *src_c, const float *src_r, cf *dst, int conj_out = 1, int rows = 1, size_t in_stride = 0);
static int forward_fft(mfb_ctx *c, const cf *src_c, const float *src_r, cf *dst, int conj_out, int rows, size_t in_stride) {
    if (!(c->use_z2 ? c->z2_rows : c->z_rows)) return MFB_ERR_STATE;       // the transforms' intermediate arrives with the filters
    if (rows < 1 || (size_t)rows > (c->use_z2 ? c->z2_rows : c->z_rows) || in_stride > 0x7fffffffu) return MFB_ERR_ARG;
    P1Args a = p1_base(c);
    a.X = src_c;
    a.Xr = src_r;
    a.ntiles = c->N2 / TILE;
    a.mgroups = 1;
    a.jsplit = rows;
    a.in_stride = (int)in_stride;
    dim3 g1(a.ntiles * rows, 1, 1);
    int rc = src_c ? launch_p1<KIND_FWDC>(c, a, g1) : launch_p1<KIND_FWDR>(c, a, g1);
    if (rc) return rc;
    P2Args b = p2_base(c);
    p2_store_split(c, b, 1);
    dim3 g2(b.parts, rows, 1);
    rc = launch_p2<MODE_STORE>(c, b, g2);
    if (rc) return rc;
    return launch_transpose(c, dst, rows, conj_out);   // conj_out = 0 leaves conj(fft(src)) (real input only)
}


// ---- single-pass overlap-save launches -------------------------------------------------------------
static int launch_seg(mfb_ctx *c, const SegArgs &a, const SegPlan &p, int mode, int pv) {
    const int rc = visit_seg([&](auto k) -> int {
        using K = decltype(k);
        if (K::SEGL != c->segl || K::MODE != mode || K::PV != pv) return VISIT_NEXT;
        hipLaunchKernelGGL((k_seg<K::L, K::MODE, K::PV>), dim3(p.grid), dim3(SegCfg<K::L>::BLOCK), (size_t)p.lds_bytes, c->stream, a);
        HIPCHK(hipGetLastError());
        return MFB_OK;
    }, SegLens{});
    return rc == VISIT_NEXT ? MFB_ERR_UNSUPPORTED : rc;
}

static SegArgs seg_base(mfb_ctx *c, const SegPlan &p) {
    SegArgs a;
    memset(&a, 0, sizeof(a));
    a.x = c->d_in;
    a.G = c->d_G;
    a.Grows = c->M;
    a.twL = c->d_twL;
    a.twLo = c->d_twLo;
    a.twHi = c->d_twHi;
    a.N = c->N;
    a.lo = c->lo;
    a.V = c->V;
    a.mpb = p.mpb;
    a.mgroups = p.mgroups;
    a.igroups = p.igroups;
    a.nsg = p.nsg;
    a.bsplit = p.bsplit;
    a.ssplit = p.ssplit;
    a.scale = 1.0f / 262144.0f;
    return a;
}

#define MIRROR_MAX_N (1 << 18)
// d_X is about to be overwritten: the copy of the previous spectrum must have left it
static int before_fft(mfb_ctx *c) {
    if (c->mirror_valid) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_X, 0));
    c->mirror_valid = false;
    return MFB_OK;
}
// d_X holds a new spectrum: start its copy to the host mirror beside whatever the handle's stream does next
static int after_fft(mfb_ctx *c) {
    if (!c->mirror) return MFB_OK;
    HIPCHK(hipEventRecord(c->ev_fft, c->stream));
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->ev_fft, 0));
    HIPCHK(hipMemcpyAsync(c->h_X, c->d_X, (size_t)c->N * sizeof(cf), hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipEventRecord(c->ev_X, c->copy_stream));
    c->mirror_valid = true;
    return MFB_OK;
}
static int enable_mirror(mfb_ctx *c) {
    if (c->mirror || c->N > MIRROR_MAX_N) return MFB_OK;
    if (!c->h_X) HIPCHK(c->h_X.alloc((size_t)c->N * sizeof(cf), hip_host_malloc));
    if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(out(c->copy_stream), hipStreamNonBlocking));
    if (!c->ev_fft) HIPCHK(hipEventCreateWithFlags(out(c->ev_fft), hipEventDisableTiming));
    if (!c->ev_X) HIPCHK(hipEventCreateWithFlags(out(c->ev_X), hipEventDisableTiming));
    c->mirror = true;
    return MFB_OK;
}

// ---- integer IQ samples (unpack_kernels.hpp) ---------------------------------------------------------------------------------
static int fmt_bytes(int fmt) { return fmt == MFB_SAMPLES_SC16 ? 4 : fmt == MFB_SAMPLES_SC8 ? 2 : (int)sizeof(cf); }
// The value of one integer step: 0 = full scale 1.0 (2^-15 / 2^-7), else a positive power of two that keeps every product a normal
// float -- the whole reason the conversion is exact (include/mfbank.h).  Returns 0 for anything else.
static float fmt_scale_checked(int fmt, float scale) {
    if (scale == 0.f) return fmt == MFB_SAMPLES_SC16 ? 0x1p-15f : 0x1p-7f;
    int e = 0;
    if (!(scale > 0.f) || isinf(scale) || frexpf(scale, &e) != 0.5f) return 0.f;
    const float top = scale * (fmt == MFB_SAMPLES_SC16 ? 32768.f : 128.f);
    if (scale < 0x1p-126f || isinf(top)) return 0.f;
    return scale;
}
static int launch_unpack(int fmt, const void *raw, cf *dst, size_t samples, float scale, hipStream_t s) {
    const dim3 grid((unsigned)unpack_blocks(fmt, samples)), block(UNPACK_THREADS);
    if (fmt == MFB_SAMPLES_SC16) hipLaunchKernelGGL(k_unpack<UNPACK_SC16>, grid, block, 0, s, raw, (float2 *)dst, samples, scale);
    else hipLaunchKernelGGL(k_unpack<UNPACK_SC8>, grid, block, 0, s, raw, (float2 *)dst, samples, scale);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}
// `samples` raw samples of a page-locked input to its staging buffer `rawslot` and, right behind the copy on the same stream,
// as complex64 into dst.  The staging buffer is made (or grown: everything that may read the old one is waited for) here.
static int raw_copy_unpack(mfb_ctx *c, const void *src, cf *dst, size_t samples, int rawslot, hipStream_t s) {
    const size_t bytes = samples * (size_t)fmt_bytes(c->fmt), need = (bytes + 15) & ~(size_t)15;
    if (c->raw_cap[rawslot] < need) {
        if (c->d_raw[rawslot]) {
            HIPCHK(sync_streams(c));
            if (c->in_stream) HIPCHK(hipStreamSynchronize(c->in_stream));
        }
        const int rc = grow_buffers(&c->raw_cap[rawslot], need, {{&c->d_raw[rawslot], need}});
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(c->d_raw[rawslot], src, bytes, hipMemcpyHostToDevice, s));
    return launch_unpack(c->fmt, c->d_raw[rawslot], dst, samples, c->fmt_scale, s);
}

extern "C" int mfb_upload(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->fmt != MFB_SAMPLES_CF32) {
        const int rc = raw_copy_unpack(c, c->h_in, c->d_x, (size_t)c->N, 0, c->stream);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(c->d_x, c->h_in, (size_t)c->N * sizeof(cf), hipMemcpyHostToDevice, c->stream));
    }
    c->d_in = c->d_x;
    int rc = before_fft(c);
    if (rc) return rc;
    rc = forward_fft(c, c->d_in, nullptr, c->d_X);
    if (rc) return rc;
    if ((rc = after_fft(c))) return rc;
    c->have_input = true;
    c->have_xc = false;
    return MFB_OK;
}

extern "C" int mfb_upload_from(mfb_ctx *c, const float *host, int N) {
    if (!c || !host || N != c->N) return MFB_ERR_ARG;
    if (c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_UNSUPPORTED;      // complex64 host data; the pinned buffer holds integers
    if ((const void *)host != (const void *)c->h_in) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(sync_streams(c));  // pinned buffer may still be in flight
        memcpy(c->h_in, host, (size_t)N * sizeof(cf));
    }
    return mfb_upload(c);
}

extern "C" int mfb_upload_device(mfb_ctx *c, const void *dev) {
    if (!c || !dev) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    c->d_in = (const cf *)dev;
    int rc = before_fft(c);
    if (rc) return rc;
    rc = forward_fft(c, c->d_in, nullptr, c->d_X);
    if (rc) return rc;
    if ((rc = after_fft(c))) return rc;
    c->have_input = true;
    c->have_xc = false;
    return MFB_OK;
}

// ---- the search with the shift on the filter side (seg_kernels.hpp, segf_body) ------------------------------------------------------
// per-bin spectra of the bank in force (the unique filters, or the span basis), built when the shifts or the filters have changed
static int fsm_prepare(mfb_ctx *c, const SearchPlan &plan) {
    const int span = plan.need_span, rows = plan.need_rows, wkt = plan.need_wkt;
    if (c->d_Gs && c->gs_rows == rows && c->gs_span == span && c->gs_l == c->segl && c->wb_kt == wkt) return MFB_OK;
    if ((int)c->h_shifts.size() != c->Dtot || !c->bank) return MFB_ERR_STATE;
    std::vector<float> G, Q;
    std::vector<uint16_t> W;
    std::vector<int> Wexp;
    // SUM_ALL searches: the per-bin table of sum_rows w |G|^2 (segf_body, SUMQ); w = how often k_finalize counts the row, relative to
    // row 0, whose partial sums carry the bin's total
    std::vector<float> *q = (c->sum_all && MFB_SEG_SUMQ) ? &Q : nullptr;
    const int L = 1 << c->segl, Te = c->T;
    if (span) {
        taps::Bank sb;
        if (taps::span_basis(*c->bank, &sb) != rows) return MFB_ERR_STATE;
        taps::segment_spectra_shifted(sb, nullptr, rows, c->h_shifts.data(), c->Dtot, L, Te, &G, seg_ppl(L), q, nullptr);
        if (wkt) taps::wrap_taps_shifted(sb, nullptr, rows, c->h_shifts.data(), c->Dtot, wkt, &W, &Wexp);
    } else {
        if ((int)c->h_uniq.size() != rows || (int)c->h_mult.size() != rows || c->h_mult[0] < 1) return MFB_ERR_STATE;
        std::vector<double> wts((size_t)rows);
        for (int u = 0; u < rows; ++u) wts[(size_t)u] = (double)c->h_mult[(size_t)u] / (double)c->h_mult[0];
        taps::segment_spectra_shifted(*c->bank, c->h_uniq.data(), rows, c->h_shifts.data(), c->Dtot, L, Te, &G, seg_ppl(L), q, wts.data());
        if (wkt) taps::wrap_taps_shifted(*c->bank, c->h_uniq.data(), rows, c->h_shifts.data(), c->Dtot, wkt, &W, &Wexp);
    }
    HIPCHK(sync_streams(c));
    c->gs_rows = 0;
    c->wb_kt = 0;
    HIPCHK(c->d_Gs.reset());
    HIPCHK(c->d_Qs.reset());
    HIPCHK(c->d_Wb.reset());
    HIPCHK(c->d_Wexp.reset());
    HIPCHK(c->d_Gs.alloc(G.size() * sizeof(float), dev_alloc));
    HIPCHK(hipMemcpy(c->d_Gs, G.data(), G.size() * sizeof(float), hipMemcpyHostToDevice));
    if (q) {
        HIPCHK(c->d_Qs.alloc(Q.size() * sizeof(float), dev_alloc));
        HIPCHK(hipMemcpy(c->d_Qs, Q.data(), Q.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (wkt) {
        HIPCHK(c->d_Wb.alloc(W.size() * sizeof(uint16_t), dev_alloc));
        HIPCHK(hipMemcpy(c->d_Wb, W.data(), W.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(c->d_Wexp.alloc(Wexp.size() * sizeof(int), dev_alloc));
        HIPCHK(hipMemcpy(c->d_Wexp, Wexp.data(), Wexp.size() * sizeof(int), hipMemcpyHostToDevice));
        c->wb_kt = wkt;
    }
    c->gs_rows = rows;
    c->gs_span = span;
    c->gs_l = c->segl;
    return MFB_OK;
}
// the complete slots of nb blocks through k_segf / k_segw, as planned; the caller has the partial sums reserved
static int launch_fsm(mfb_ctx *c, const SearchPlan &p, int nb, const cf *x, int xstride) {
    // fsm_prepare built the bin tables for this plan; tables that do not match it are an error, not a reason to run another form
    const bool tables = c->d_Gs && c->gs_rows == p.need_rows && c->gs_span == p.need_span && c->gs_l == p.need_segl && c->wb_kt == p.need_wkt &&
                        (!p.sumq || c->d_Qs) && (!p.need_wkt || (c->d_Wb && c->d_Wexp));
    if (!tables || (p.form == SEARCH_SEGW && (p.sumq != 2 || p.pv != SEGW_PV))) return MFB_ERR_STATE;
    SegFArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x, a.xstride = xstride, a.nblk = nb, a.dper = c->Dtot;
    a.Gs = c->d_Gs, a.twL = c->d_twL;
    a.Qs = c->sum_all ? c->d_Qs : nullptr;
    a.presum = p.presum;
    a.partials = c->d_part, a.part_row0 = 0, a.parts = p.parts;
    a.N = c->N, a.V = c->V, a.MU = p.rows;
    a.slot0 = 0, a.nslots = p.nfull;
    a.nsg = p.nsg, a.gbins = p.gbins, a.fb = p.fb, a.fs = p.fs, a.nbc = p.nbc, a.nsc = p.nsc;
    a.scale = 1.0f / 262144.0f;
    // the wrap-around energy on the matrix cores (wrap_kernels.hpp)
    if (p.form == SEARCH_SEGW) {
        const SegWArgs w = {a, c->d_Wb, c->d_Wexp, c->bank->T};
        hipLaunchKernelGGL((k_segw<SEGW_PV, SEGW_KT>), dim3(p.grid), dim3(SegCfg<256>::BLOCK), (size_t)p.lds_bytes, c->stream, w);
        HIPCHK(hipGetLastError());
        return MFB_OK;
    }
    const int rc = visit_segf([&](auto k) -> int {
        using K = decltype(k);
        if (K::SEGL != p.segl || K::PV != p.pv || K::MODE != p.sumq) return VISIT_NEXT;
        hipLaunchKernelGGL((k_segf<K::L, K::PV, K::MODE>), dim3(p.grid), dim3(SegCfg<K::L>::BLOCK), (size_t)p.lds_bytes, c->stream, a);
        HIPCHK(hipGetLastError());
        return MFB_OK;
    });
    return rc == VISIT_NEXT ? MFB_ERR_UNSUPPORTED : rc;
}

// Build the per-bin spectra as soon as filters, shifts and the path are known (mfb_set_filters / mfb_set_shifts / mfb_set_search_*),
// not inside the first search: 512 transforms of 2048 points for the 384-tap bank at 64 bins are 10-20 ms of host work, which does
// not belong into a receive loop's first block.  (The search still checks, and builds what is missing.)
static int fsm_prepare_eager(mfb_ctx *c) {
    if (!c->have_filters || !c->have_shifts || c->path != MFB_PATH_SEGMENT) return MFB_OK;
    const SearchPlan p = plan_search(search_inputs(c), segments(c), 1);
    return p.need_tables ? fsm_prepare(c, p) : MFB_OK;
}
// how the segment search of the next block will run: filter_side = 1 when the Doppler shift sits on the filters' side (k_segf: one
// forward transform per segment for `bins_per_forward` bins), 0 when every (bin, segment) is mixed and transformed (k_seg)
extern "C" int mfb_get_search_info(mfb_ctx *c, int *filter_side, int *bins_per_forward) {
    if (!c || !filter_side || !bins_per_forward) return MFB_ERR_ARG;
    const bool planned = c->path == MFB_PATH_SEGMENT && c->have_filters;
    const SearchPlan p = planned ? plan_search(search_inputs(c), segments(c), 1) : SearchPlan{};
    *filter_side = p.need_tables;
    *bins_per_forward = p.need_tables ? p.fb : 1;
    return MFB_OK;
}
extern "C" int mfb_debug_search_plan(mfb_ctx *c, mfb_plan_inputs *inputs, int nblocks, mfb_search_plan *out) {
    if (!inputs || !out || nblocks < 1) return MFB_ERR_ARG;
    if (c && !c->have_filters) return MFB_ERR_STATE;
    if (c) *inputs = search_inputs(c);
    const Segments sg = c ? segments(c) : resolve_segments(*inputs);
    if (!sg.ok) return MFB_ERR_UNSUPPORTED;
    *out = plan_search(*inputs, sg, nblocks);
    if (sg.path == MFB_PATH_SEGMENT) out->store = plan_store(*inputs, sg, nblocks);     // ... and the matched-filter pass of the same blocks
    return MFB_OK;
}

// The segment-path search of nb blocks in ONE launch (+ the masked tail launch + k_finalize): stream jl of the launch is bin
// jl % Dtot of block jl / Dtot, block b's samples start at x + b * xstride, its doppSum rows at dsum + b * Dtot * M.  nb = 1 is
// the plain search of one block.  A score depends on the block, the shift and the filter only (seg_kernels.hpp), so a
// block's rows come out bit for bit the same whichever batch it is part of.
static int seg_search_enqueue(mfb_ctx *c, int nb, const cf *x, int xstride, float *dsum) {
    const SearchPlan p = plan_search(search_inputs(c), segments(c), nb);     // every decision of this search, taken once
    const bool span = p.basis == MFB_BASIS_SPAN;
    const int MU = p.rows, rows = nb * c->Dtot;      // filters transformed per bin, Doppler streams of the launch
    int rc = reserve_partials(c, (size_t)rows * MU * p.parts);
    if (rc) return rc;
    if (p.need_tables && (rc = fsm_prepare(c, p))) return rc;       // (built by the first block: nothing is allocated inside a graph capture)
    auto seg_args = [&](const SegPlan &sp, int slot0, int nslots) {
        SegArgs a = seg_base(c, sp);
        if (span) a.G = c->d_Gb, a.Grows = c->MB;
        a.x = x, a.shifts = c->d_shifts, a.partials = c->d_part;
        a.rows = (!span && MU < c->M) ? c->d_uniq : nullptr;
        a.MU = MU, a.dc = rows, a.parts = p.parts;
        if (nb > 1) a.dper = c->Dtot, a.xstride = xstride;
        a.slot0 = slot0, a.nslots = nslots;
        return a;
    };
    prof_mark(c, 0);
    // (both roles inside one grid were tried: the merged kernel ran 8-10 % slower than two launches)
    if (p.need_tables) rc = launch_fsm(c, p, nb, x, xstride);
    else if (p.form == SEARCH_SEG) rc = launch_seg(c, seg_args(p.main_seg, 0, p.nfull), p.main_seg, SEG_REDUCE, p.pv);
    if (!rc && p.ntotal > p.nfull) rc = launch_seg(c, seg_args(p.tail, p.nfull, p.ntotal - p.nfull), p.tail, SEG_REDUCE, -1);
    if (rc) return rc;
    prof_mark(c, 0);
    // the forms that sum a bin's rows in registers store row 0 alone: rows >= 1 hold the masked tail's partials and nothing else
    const int row0_only = p.need_tables && p.sumq == 2;
    hipLaunchKernelGGL(k_finalize, dim3(rows), dim3(fin_threads(MU)), 0, c->stream, c->d_part, dsum, rows, c->M, MU,
                       span ? (const int *)nullptr : (const int *)c->d_rep, p.parts, c->sum_all, row0_only, p.nfull * seg_geom(p.segl).WPT);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}

extern "C" int mfb_search_async(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    if (!c->have_filters || !c->have_shifts || !c->have_input) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const int MU = c->MU;
    if (c->search_mode == MFB_SEARCH_ENERGY) {
        // opt-in shortcut (energy_kernels.hpp): no transform, D.N multiply-adds on |X|^2 and the filters' energy
        const int R = c->sum_all ? 1 : c->M;
        const int parts = c->N / EN_CHUNK;
        int rc = reserve_partials(c, (size_t)c->Dtot * R * parts);
        if (rc) return rc;
        if (!c->d_pow) HIPCHK(c->d_pow.alloc((size_t)c->N * sizeof(float), dev_alloc));
        if (!c->d_W) HIPCHK(c->d_W.alloc((size_t)c->N * (c->sum_all ? 1 : c->M) * sizeof(float), dev_alloc));
        if (!c->W_valid) {
            hipLaunchKernelGGL(k_filter_energy, dim3(c->N / 256, R), dim3(256), 0, c->stream, (const cf *)c->d_masks, c->d_W, c->N, c->M,
                               c->sum_all);
            HIPCHK(hipGetLastError());
            c->W_valid = true;
        }
        prof_mark(c, 0);
        hipLaunchKernelGGL(k_power, dim3(c->N / 256), dim3(256), 0, c->stream, (const cf *)c->d_X, c->d_pow, c->N);
        hipLaunchKernelGGL(k_energy, dim3(parts, R), dim3(256), 0, c->stream, (const float *)c->d_pow, (const float *)c->d_W,
                           (const int *)c->d_shifts, c->d_part, c->N, c->Dtot, R, parts, (float)c->N / 262144.f);
        HIPCHK(hipGetLastError());
        prof_mark(c, 0);
        hipLaunchKernelGGL(k_finalize, dim3(c->Dtot), dim3(fin_threads(R)), 0, c->stream, c->d_part, c->d_sum, c->Dtot, c->M, R, (const int *)nullptr,
                           parts, c->sum_all, 0, 0);
        HIPCHK(hipGetLastError());
        return MFB_OK;
    }
    if (c->path == MFB_PATH_SEGMENT) return seg_search_enqueue(c, 1, c->d_in, 0, c->d_sum);
    const int mpb = c->mpb < MU ? c->mpb : MU;
    const int mgroups = (MU + mpb - 1) / mpb;
    for (int j0 = 0; j0 < c->Dtot; j0 += c->chunk) {
        const int dc = (c->Dtot - j0) < c->chunk ? (c->Dtot - j0) : c->chunk;
        P1Args a = p1_base(c);
        a.X = c->d_X;
        a.shifts = c->d_shifts;
        a.j0 = j0;
        a.dc = dc;
        a.M = MU;
        a.mpb = mpb;
        a.rows = (MU < c->M) ? c->d_uniq : nullptr;
        const int js = c->jsplit < dc ? c->jsplit : dc;
        a.ntiles = c->N2 / TILE;
        a.mgroups = mgroups;
        a.jsplit = js;
        prof_mark(c, 0);
        int rc = launch_p1<KIND_BANK>(c, a, dim3(a.ntiles * mgroups * js, 1, 1));
        prof_mark(c, 0);
        if (rc) return rc;
        P2Args b = p2_base(c);
        b.partials = c->d_part;
        b.part_row0 = j0 * MU;
        prof_mark(c, 1);
        rc = launch_p2<MODE_REDUCE>(c, b, dim3(c->parts, dc * MU, 1));
        prof_mark(c, 1);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_finalize, dim3(c->Dtot), dim3(fin_threads(MU)), 0, c->stream, c->d_part, c->d_sum, c->Dtot, c->M, MU,
                       (const int *)c->d_rep, c->parts, c->sum_all, 0, 0);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}

// device -> host through the page-locked landing zone when it fits (n pieces back to back, ONE synchronisation)
struct BackPiece {
    void *host;
    const void *dev;
    size_t bytes;
};
static int read_back(mfb_ctx *c, const BackPiece *p, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (p[i].bytes + 15) & ~(size_t)15;
    const bool staged = c->h_back && total <= c->back_cap;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (!p[i].bytes) continue;
        HIPCHK(hipMemcpyAsync(staged ? (void *)(c->h_back + off) : p[i].host, p[i].dev, p[i].bytes, hipMemcpyDeviceToHost, c->stream));
        off += (p[i].bytes + 15) & ~(size_t)15;
    }
    HIPCHK(sync_streams(c));
    if (staged) {
        off = 0;
        for (int i = 0; i < n; ++i) {
            if (p[i].bytes) memcpy(p[i].host, c->h_back + off, p[i].bytes);
            off += (p[i].bytes + 15) & ~(size_t)15;
        }
    }
    return MFB_OK;
}

extern "C" int mfb_export_scores_async(mfb_ctx *c, void *dst, int row_offset) {
    if (!c || !dst || row_offset < 0) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync((float *)dst + (size_t)row_offset * c->M, c->d_sum, (size_t)c->Dtot * c->M * sizeof(float),
                          hipMemcpyDeviceToDevice, c->stream));
    return MFB_OK;
}

extern "C" int mfb_export_column_async(mfb_ctx *c, void *dst, int row_offset) {
    if (!c || !dst || row_offset < 0) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    // column 0 of doppSum [Dtot][M] -> dst[row_offset + j]
    HIPCHK(hipMemcpy2DAsync((float *)dst + row_offset, sizeof(float), c->d_sum, (size_t)c->M * sizeof(float), sizeof(float),
                            (size_t)c->Dtot, hipMemcpyDeviceToDevice, c->stream));
    return MFB_OK;
}

extern "C" int mfb_export_rows_async(mfb_ctx *c, void *dst, int dst_row, int first_row, int nrows, int column_only) {
    if (!c || !dst || dst_row < 0 || first_row < 0 || nrows < 0 || first_row + nrows > c->Dtot) return MFB_ERR_ARG;
    if (!nrows) return MFB_OK;
    HIPCHK(hipSetDevice(c->device));
    const float *src = c->d_sum + (size_t)first_row * c->M;
    if (column_only)
        HIPCHK(hipMemcpy2DAsync((float *)dst + dst_row, sizeof(float), src, (size_t)c->M * sizeof(float), sizeof(float), (size_t)nrows,
                                hipMemcpyDeviceToDevice, c->stream));
    else
        HIPCHK(hipMemcpyAsync((float *)dst + (size_t)dst_row * c->M, src, (size_t)nrows * c->M * sizeof(float), hipMemcpyDeviceToDevice,
                              c->stream));
    return MFB_OK;
}

// The pick k_pick has just been asked for (pick number c->picks), from the handle's page-locked slot: the kernel stores it there
// itself, and the host takes it when it arrives -- hipStreamSynchronize returns only after the end-of-kernel release, the completion
// signal and the runtime's wake-up, and the device stands empty meanwhile.  The slot is the pick's when its number is c->picks and its
// check word fits the two floats (k_pick): the pick before, or a store seen in pieces, is waited out.  The wait is bounded: after
// PICK_SPIN_US, or as soon as the stream is anything but busy (finished without the store having been seen, or failed), it ends in
// the synchronise it always ended in, with that call's errors; so does a pick with work on the batch path's second stream, which
// that synchronise waits for too.  The stream is in order, so a pick that has arrived says that everything ahead of k_pick is
// complete; only k_pick's own end may still be pending, and nothing the host does next depends on that (mfb_destroy, the reserve
// paths, mfb_set_stream, the timer and every other read-back synchronise for themselves).
static constexpr int PICK_SPIN_US = 800;
static int read_pick(mfb_ctx *c, float res[2]) {
    const uint32_t want = c->picks;
    const volatile uint32_t *slot = c->h_pick.get();
    auto arrived = [&] {
        const uint32_t w0 = slot[0], w1 = slot[1], w2 = slot[2], w3 = slot[3];
        if (w2 != want || w3 != (want ^ w0 ^ w1)) return false;
        memcpy(&res[0], &w0, sizeof(float));
        memcpy(&res[1], &w1, sizeof(float));
        return true;
    };
    if (!(c->s2 && c->s2_busy)) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 1;; ++spin) {
            if (arrived()) return MFB_OK;
            mfb_cpu_relax();
            if ((spin & 255u) == 0u) {
                if (hipStreamQuery(c->stream) != hipErrorNotReady) break;
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(PICK_SPIN_US)) break;
            }
        }
    }
    HIPCHK(sync_streams(c));
    return arrived() ? MFB_OK : MFB_ERR_HIP;       // (a kernel that ended without its store: never seen; not a pick to hand out)
}

extern "C" int mfb_pick_column(mfb_ctx *c, const void *column, int num, int offset, float res[2]) {
    if (!c || !column || !res || num < 1 || offset < 0) return MFB_ERR_ARG;
    if (!c->sum_all) return MFB_ERR_STATE;   // a single column is the whole table only under SUM_ALL_MASKS
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_pick, dim3(1), dim3(64), 0, c->stream, (const float *)column, c->d_res, c->h_pick_dev, ++c->picks, num, offset, 1, 1);
    HIPCHK(hipGetLastError());
    return read_pick(c, res);
}

extern "C" int mfb_pick(mfb_ctx *c, const void *scores, int num, int offset, float res[2]) {
    if (!c || !res || num < 1 || offset < 0) return MFB_ERR_ARG;
    if (!scores && (num != c->D || offset != c->Doff)) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const float *in = scores ? (const float *)scores : c->d_sum;
    hipLaunchKernelGGL(k_pick, dim3(1), dim3(64), 0, c->stream, in, c->d_res, c->h_pick_dev, ++c->picks, num, offset, c->M, c->sum_all);
    HIPCHK(hipGetLastError());
    return read_pick(c, res);
}

extern "C" int mfb_find_carrier(mfb_ctx *c, float res[2]) {
    int rc = mfb_search_async(c);
    if (rc) return rc;
    return mfb_pick(c, nullptr, c->D, c->Doff, res);
}

extern "C" int mfb_get_scores(mfb_ctx *c, float *host) {
    if (!c || !host) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(host, c->d_sum, (size_t)c->Dtot * c->M * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    return MFB_OK;
}

// doppSum of block `block` of the LAST batch (mfb_receive_blocks_*), as mfb_get_scores gives the one-block table
extern "C" int mfb_get_batch_scores(mfb_ctx *c, int block, float *host) {
    if (!c || !host || block < 0) return MFB_ERR_ARG;
    if (!c->d_sumb || block >= c->bat_cap || block >= c->last_batch_blocks) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    HIPCHK(hipMemcpy(host, c->d_sumb + (size_t)block * c->Dtot * c->M, (size_t)c->Dtot * c->M * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

extern "C" int mfb_get_spectrum(mfb_ctx *c, float *host, int start, int count) {
    if (!c || !host || count < 0 || count > c->N) return MFB_ERR_ARG;
    if (!c->have_input) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    start = ((start % c->N) + c->N) % c->N;
    const int first = (start + count <= c->N) ? count : c->N - start;
    if (c->mirror_valid) {            // the spectrum is (or is about to be) on the host already
        HIPCHK(hipEventSynchronize(c->ev_X));
        memcpy(host, c->h_X + start, (size_t)first * sizeof(cf));
        if (first < count) memcpy(host + 2 * (size_t)first, c->h_X, (size_t)(count - first) * sizeof(cf));
        return MFB_OK;
    }
    const BackPiece bp[2] = {{host, c->d_X + start, (size_t)first * sizeof(cf)},
                             {host + 2 * (size_t)first, c->d_X, (size_t)(count - first) * sizeof(cf)}};
    const int rc = read_back(c, bp, 2);
    if (rc) return rc;
    return enable_mirror(c);          // a caller that reads the spectrum once will read it again after every block
}

// Where a block -- or a batch of nb blocks -- lives on the device while it goes through the block path.
struct BlkBufs {
    int nb;              // blocks
    const cf *x;         // samples: block b starts at x + b * xstride
    int xstride;
    cf *X;               // spectra [nb][N]
    float *sum;          // doppSum [nb][Dtot][M]
    float *res;          // picks [nb][2]
    cf *xc;              // matched-filter outputs [nb][M][N]
    float *env;          // symbol-energy envelopes [nb][N]
    cf *P;               // their spectra [nb][N]
    float *cr;           // rate triples [nb][3]
    uint8_t *out;        // result records [nb][lay.bytes]
    RecordLayout lay;    // (lay.stages: the stream stages run on the device, behind the centres)
    bool batch;          // mfb_receive_blocks_*: the handle's one-block state (d_in, have_input, mirror) stays out of it
    int parity;          // carry buffer the stream stages read
    const struct ClipLaunch *clip;   // peak clip in front of the forward transform (nullptr: none); x is then its output
};
static BlkBufs single_bufs(mfb_ctx *c, const RecordLayout &lay = RecordLayout{}) {
    return BlkBufs{1, c->d_in, 0, c->d_X, c->d_sum, c->d_res, c->d_xc, c->d_env, c->d_P, c->d_cr, c->d_blkout, lay, false, 0, nullptr};
}

// A9 + A10 enqueued on the handle's stream: matched filters at one shift per block (a value, or -- shift_dev != nullptr -- an
// int the device has just computed; for a batch, block b's sits shift_stride ints behind block b - 1's), envelope, its
// spectrum, windowed argmax into cr.  No synchronisation.
static int demod_enqueue(mfb_ctx *c, const BlkBufs &bb, int shift, const int *shift_dev, int shift_stride, int k_offset, int k_len,
                         int spsym_min = 0, int capacity = 0, BlockScalars *scal = nullptr) {
    // A9: matched filters at one shift -> xc[M][N] natural order
    int rc;
    const int nb = bb.nb;
    if (c->path == MFB_PATH_SEGMENT) {
        // the same segment kernel, storing y in natural order instead of reducing it (no transpose)
        // one bin: spread the slots over the chip.  When a team takes all M filters of its segments (M <= 16) it also
        // sums the symbol-energy envelope (sumXCorrBuffMasks, CU:191-205) in the same pass; otherwise the filters are
        // spread too and k_envelope follows (plan_store)
        const bool fused_env = c->M <= SEG_MPB_MAX;
        const SegPlan p = plan_store(search_inputs(c), segments(c), nb);
        int nfull, ntotal;
        seg_slots(c->N, segments(c), &nfull, &ntotal);
        SegArgs sa = seg_base(c, p);
        sa.x = bb.x;
        sa.out = bb.xc;
        if (fused_env) {
            sa.env = bb.env;
            sa.env_lo = c->cs_off;
            sa.env_hi = c->M - c->cs_off;
        }
        sa.MU = c->M;
        sa.dc = nb;
        sa.slot0 = 0;
        sa.nslots = ntotal;
        sa.shifts = shift_dev;
        sa.j0 = 0;
        sa.fixed_shift = shift;
        sa.out_off = (c->win_start + c->T - 1) & (c->N - 1);
        if (nb > 1) {
            sa.dper = 1;
            sa.xstride = bb.xstride;
            sa.sstride = shift_stride;
            sa.ostride = (long long)c->M * c->N;
        }
        rc = launch_seg(c, sa, p, SEG_STORE, -1);
        if (rc) return rc;
    } else {
        if (nb != 1) return MFB_ERR_UNSUPPORTED;        // batches of blocks run on the segment path
        P1Args a = p1_base(c);
        a.X = bb.X;
        a.shifts = shift_dev;
        a.j0 = 0;
        a.fixed_shift = shift;
        a.dc = 1;
        const int mgroups = (c->M + c->mpb - 1) / c->mpb;
        a.ntiles = c->N2 / TILE;
        a.mgroups = mgroups;
        a.jsplit = 1;
        rc = launch_p1<KIND_BANK>(c, a, dim3(a.ntiles * mgroups, 1, 1));
        if (rc) return rc;
        P2Args b = p2_base(c);
        p2_store_split(c, b, c->M);
        rc = launch_p2<MODE_STORE>(c, b, dim3(b.parts, c->M, 1));
        if (rc) return rc;
        rc = launch_transpose(c, bb.xc, c->M, 0);
        if (rc) return rc;
    }
    // A10: envelope (unless the matched-filter launch already summed it), spectrum of the envelope, windowed argmax
    if (!(c->path == MFB_PATH_SEGMENT && c->M <= SEG_MPB_MAX)) {
        hipLaunchKernelGGL(k_envelope, dim3(1024, nb), dim3(256), 0, c->stream, (const cf *)bb.xc, bb.env, c->N, c->M, c->cs_off);
        HIPCHK(hipGetLastError());
    }
    rc = forward_fft(c, nullptr, bb.env, bb.P, 1, nb, (size_t)c->N);
    if (rc) return rc;
    if (scal)
        hipLaunchKernelGGL(k_code_rate_block, dim3(nb), dim3(1024), 0, c->stream, (const cf *)bb.P, bb.cr, k_offset, k_len, c->N, spsym_min,
                           capacity, scal, bb.lay.bytes);
    else
        hipLaunchKernelGGL(k_code_rate, dim3(1), dim3(1024), 0, c->stream, (const cf *)bb.P, bb.cr, k_offset, k_len);
    HIPCHK(hipGetLastError());
    return MFB_OK;
}

extern "C" int mfb_demodulate(mfb_ctx *c, int shift, int k_offset, int k_len, float res[3]) {
    if (!c || !res) return MFB_ERR_ARG;
    if (!c->have_filters || !c->have_input) return MFB_ERR_STATE;
    if (k_offset < 0 || k_len < 0 || k_offset + k_len > c->N) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    shift = ((shift % c->N) + c->N) % c->N;
    int rc = demod_enqueue(c, single_bufs(c), shift, nullptr, 0, k_offset, k_len);
    if (rc) return rc;
    const BackPiece bp = {res, c->d_cr, 3 * sizeof(float)};
    if ((rc = read_back(c, &bp, 1))) return rc;
    c->have_xc = true;
    return MFB_OK;
}

// ---- one call per block --------------------------------------------------------------------------------------------
// Everything the receive loop does with one block on the device (reference demodulator_base.py:548-632 and 711-1009), as ONE
// stream of launches and ONE synchronisation: [H2D of the pinned input buffer,] forward FFT, Doppler search, pick, shift
// interpolation (k_block_pick), the two spectrum windows of computeSNR, matched filters at that shift, envelope, its
// spectrum, rate/phase argmax, the float64 arithmetic behind it (k_block_rate), symbol centres -- then one packed read-back.
// The same launches take a BATCH of bb.nb consecutive blocks of one window of samples (mfb_receive_blocks_*): every kernel
// gets a block index in its grid, nothing else changes -- a block's numbers are those of the one-block call, bit for bit.
// The launches of one block / batch, from the forward FFT to the ONE device-to-host copy of the result record(s).
// A14 for the blocks of a batch: one packed launch (search + would-be stash edges + ring) where the templates allow it
static void stream_search_launch(mfb_ctx *c, const StreamArgs &sa, int nb, int Tmax) {
    const size_t words = (size_t)((STREAM_PACK_TAPS + sa.T[0] - 1 + STREAM_EDGE_BACK + sa.nOv + sa.nsym + 31) >> 5) + STREAM_PACK_TAPS / 32 + 4;
    static const bool unpacked = getenv("MFB_STREAM_UNPACKED") != nullptr;       // (A/B switch of tools/chain_kernels.sh)
    if (sa.packed && words * 4 <= 60 * 1024 && !unpacked) {
        hipLaunchKernelGGL(k_stream_search, dim3(nb), dim3(STREAM_SEARCH_THREADS), words * 4, c->stream, sa);
        return;
    }
    hipLaunchKernelGGL(k_stream_sync, dim3(sa.K, nb), dim3(256), (size_t)Tmax + SYNC_SEG + Tmax - 1, c->stream, sa);
    hipLaunchKernelGGL(k_stream_ring, dim3(1), dim3(256), 0, c->stream, sa);
    hipLaunchKernelGGL(k_stream_edges, dim3(nb), dim3(256), 0, c->stream, sa);
}
// where the pieces of a result record sit
struct RecPtrs {
    size_t rec;
    uint8_t *d;
    BlockScalars *scal;
    cf *bands;
    int *sym, *cen;
    float *mag;
};
static RecPtrs rec_ptrs(const BlkBufs &bb) {
    uint8_t *d = bb.out;
    const RecordLayout &l = bb.lay;
    return RecPtrs{l.bytes, d, (BlockScalars *)(d + l.scalars), (cf *)(d + l.bands), (int *)(d + l.sym), (int *)(d + l.cen), (float *)(d + l.mag)};
}
// the records a launch of the stream stages works on
static void stream_records(StreamArgs &sa, uint8_t *rec0, const RecordLayout &l) {
    sa.rec0 = rec0;
    sa.rec = l.bytes;
    sa.off_sym = l.sym;
    sa.off_cen = l.cen;
    sa.off_mag = l.mag;
    sa.off_bits = l.bits;
    sa.off_cenw = l.cenw;
    sa.off_trust = l.trust;
    sa.off_post = l.post;
    sa.off_end = l.end;
    sa.off_hits = l.hits;
    sa.off_edges = l.edges;
}
// ---- interference-peak clipping (clip_kernels.hpp; reference __thresholdInput, DB:670-707) -----------------------------------
struct ClipLaunch {
    ClipArgs a;
    int32_t *h_head;     // page-locked copy of the heads, read back with the flight
};
// buffers of the clip: the flight's own (clipped blocks, indices, heads: slot `slot`, up to nb blocks -- the other slot's flight,
// pending or collected, keeps its own), the shared workspace of part 1 and the chain tail (stable addresses: captured graphs
// hold them)
static int clip_reserve(mfb_ctx *c, int slot, int nb) {
    if (nb > c->clip_cap[slot]) {
        HIPCHK(sync_streams(c));
        ++c->epoch;
        const size_t nbN = (size_t)nb * c->N, heads = (size_t)nb * CLIP_HEAD * sizeof(int);
        const int rc = grow_buffers(&c->clip_cap[slot], 0, {{&c->d_clipx[slot], nbN * sizeof(cf)}, {&c->d_clipi[slot], nbN * sizeof(int)}, {&c->d_cliph[slot], heads}});
        if (rc) return rc;
        HIPCHK(c->h_cliph[slot].alloc(heads, hip_host_malloc));
        memset(c->h_cliph[slot], 0, heads);
        c->clip_cap[slot] = nb;        // (device and host side exist)
    }
    if (nb > c->clip_ws_cap) {       // part 1 only, on the handle's stream: nothing in flight reads it after the wait
        HIPCHK(sync_streams(c));
        ++c->epoch;
        const size_t nbN = (size_t)nb * c->N;
        const int rc = grow_buffers(&c->clip_ws_cap, nb, {{&c->d_clips, (2 * nbN / CLIP_LEAF + 2 * (size_t)nb) * sizeof(float)}, {&c->d_clipw, 2 * nbN / CLIP_WAVE * sizeof(int)}});
        if (rc) return rc;
    }
    if (c->clip_ov > c->ctail_cap) {
        HIPCHK(sync_streams(c));
        ++c->epoch;
        const size_t bytes = sizeof(ClipTail) + (size_t)c->clip_ov * sizeof(cf);
        const int rc = grow_buffers(&c->ctail_cap, 0, {{&c->d_ctail, bytes}});
        if (rc) return rc;
        HIPCHK(hipMemset(c->d_ctail, 0, bytes));
        c->ctail_cap = c->clip_ov;     // (and cleared)
    }
    return MFB_OK;
}
// The clip of nb blocks (block b at raw + b * xstride) for flight `slot`: its arguments, and the chain's restart if one is due
static int clip_prepare(mfb_ctx *c, int slot, const cf *raw, long long xstride, int nb, ClipLaunch *L) {
    // (a window's batches: room for the window's blocks at once, as batch_reserve does, so that sizes 1 ... B share the buffers)
    int rc = clip_reserve(c, slot, nb > c->win_blocks ? nb : (c->win_blocks > 0 && xstride != 0 ? c->win_blocks : nb));
    if (rc) return rc;
    ClipArgs &a = L->a;
    const size_t nbN = (size_t)c->clip_ws_cap * c->N;
    a.x = (const float2 *)raw;
    a.xstride = xstride;
    a.y = (float2 *)c->d_clipx[slot].get();
    a.idx = c->d_clipi[slot];
    a.head = c->d_cliph[slot];
    a.s1 = c->d_clips;
    a.s2 = c->d_clips + nbN / CLIP_LEAF;
    a.thr = c->d_clips + 2 * nbN / CLIP_LEAF;
    a.wcnt = c->d_clipw;
    a.wflag = c->d_clipw + nbN / CLIP_WAVE;
    a.tail = c->clip_ov > 0 ? c->d_ctail : nullptr;
    a.N = c->N;
    a.ov = c->clip_ov;
    a.nb = nb;
    a.scale = c->clip_scale;
    L->h_head = c->h_cliph[slot];
    if (c->clip_restart) {       // outside any captured graph: the next block's overlap is taken as it is
        if (c->d_ctail) HIPCHK(hipMemsetAsync(c->d_ctail, 0, sizeof(int32_t), c->stream));
        c->clip_restart = false;
    }
    return MFB_OK;
}
// sum, sum again, clip, compact for every block at once; the chain in order (ov > 0); the heads to the flight's staging
static int clip_enqueue(mfb_ctx *c, const ClipLaunch &L) {
    const ClipArgs &a = L.a;
    const dim3 grid(c->N / (CLIP_WAVE * (CLIP_THREADS / 64)), a.nb);
    hipLaunchKernelGGL(k_clip_sum1, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_sum2, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_apply, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_clip_compact, grid, dim3(CLIP_THREADS), 0, c->stream, a);
    if (a.tail) hipLaunchKernelGGL(k_clip_chain, dim3(1), dim3(CLIP_CHAIN_THREADS), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(L.h_head, a.head, (size_t)a.nb * CLIP_HEAD * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return MFB_OK;
}
extern "C" int mfb_set_peak_clip(mfb_ctx *c, float scale, int overlap) {
    if (!c || !(scale >= 0.f) || isinf(scale) || overlap < 0 || overlap >= c->N) return MFB_ERR_ARG;
    if (scale > 0.f && c->N < CLIP_THREADS / 64 * CLIP_WAVE) return MFB_ERR_UNSUPPORTED;
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    ++c->epoch;                  // the recorded graphs hold the old settings
    c->clip_scale = scale;
    c->clip_ov = scale > 0.f ? overlap : 0;
    c->clip_restart = true;
    return MFB_OK;
}
extern "C" int mfb_get_peak_clip_tail(mfb_ctx *c, float *host_c64, int count, int32_t *valid) {
    if (!c || !valid || count < 0 || (count > 0 && !host_c64)) return MFB_ERR_ARG;
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    if (c->clip_ov <= 0 || !c->d_ctail || c->clip_restart) {
        *valid = 0;
        return MFB_OK;
    }
    if (count != c->clip_ov) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    HIPCHK(hipMemcpy(valid, &c->d_ctail->valid, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*valid) HIPCHK(hipMemcpy(host_c64, c->d_ctail->s, (size_t)count * sizeof(cf), hipMemcpyDeviceToHost));
    return MFB_OK;
}
extern "C" int mfb_restart_peak_clip(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    c->clip_restart = true;
    return MFB_OK;
}
extern "C" int mfb_get_block_clips(mfb_ctx *c, int slot, int block, int32_t *idx, int cap, int32_t *count) {
    if (!c || slot < 0 || slot > 1 || block < 0 || cap < 0 || !count || (cap > 0 && !idx)) return MFB_ERR_ARG;
    const BlockFlight &f = c->flight[slot];
    if (f.active || !f.clip || block >= (f.nb ? f.nb : 1)) return MFB_ERR_STATE;
    const int32_t *h = c->h_cliph[slot] + (size_t)block * CLIP_HEAD;
    const int n = h[0];
    *count = n;
    const int m = n < cap ? n : cap;
    if (m <= CLIP_HEAD - 1) {
        if (m > 0) memcpy(idx, h + 1, (size_t)m * sizeof(int32_t));
    } else {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpy(idx, c->d_clipi[slot] + (size_t)block * c->N, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return MFB_OK;
}

// Part 1 of a block / batch: forward transform(s), Doppler search, pick (or, at a fixed shift, the cleared scalars).
// How much of a block's results its record holds: the SNR windows' capacity, the symbols the caller takes at most, and every symbol
// the rate window admits (k* < k_offset + k_len  =>  count <= k_offset + k_len), bounded by that
struct BlockGeom {
    int bcap, capacity, nthreads;
};
static BlockGeom block_geom(const mfb_ctx *c, const mfb_block_params *p) {
    BlockGeom g;
    g.bcap = p->mode == MFB_BLOCK_SEARCH ? p->band_capacity : 0;
    g.capacity = p->max_symbols < c->cap ? p->max_symbols : c->cap;
    g.nthreads = p->k_offset + p->k_len + 1 < g.capacity ? p->k_offset + p->k_len + 1 : g.capacity;
    return g;
}
static int block_enqueue_p1(mfb_ctx *c, const mfb_block_params *p, const BlkBufs &bb, const BlockGeom &geo) {
    int rc;
    const int nb = bb.nb;
    const bool batch = bb.batch;
    if (!batch && p->input == MFB_INPUT_UPLOADED) {
        if (!c->have_input) return MFB_ERR_STATE;
    } else {
        if (!batch) {
            if ((rc = before_fft(c))) return rc;
        }
        if (bb.clip && (rc = clip_enqueue(c, *bb.clip))) return rc;
        if ((rc = forward_fft(c, bb.x, nullptr, bb.X, 1, nb, (size_t)bb.xstride))) return rc;
        if (!batch) {
            if ((rc = after_fft(c))) return rc;
            c->have_input = true;
            c->have_xc = false;
        }
    }
    const RecPtrs r = rec_ptrs(bb);
    if (p->mode == MFB_BLOCK_SEARCH) {
        if (batch) {
            if (c->path != MFB_PATH_SEGMENT || c->search_mode != MFB_SEARCH_TRANSFORMS) return MFB_ERR_UNSUPPORTED;
            if ((rc = seg_search_enqueue(c, nb, bb.x, bb.xstride, bb.sum))) return rc;
        } else if ((rc = mfb_search_async(c))) {
            return rc;
        }
        // (mfb_set_device_snr: no spectrum sample is copied; the windows' means go where the signal window would begin)
        hipLaunchKernelGGL(k_pick_block, dim3(nb), dim3(64), 0, c->stream, (const float *)bb.sum, bb.res, c->D, c->Doff, c->M, c->sum_all,
                           (const int *)c->d_shifts, c->Dtot, c->N, p->snr_window, (const cf *)bb.X, r.scal, r.bands,
                           c->device_snr ? 0 : geo.bcap, r.rec);
        HIPCHK(hipGetLastError());
        if (c->device_snr && geo.bcap > 0) {
            hipLaunchKernelGGL(k_band_means, dim3(2, nb), dim3(SNR_THREADS), 0, c->stream, (const float2 *)bb.X, (size_t)c->N, c->N,
                               (const int *)&r.scal->band[0][0][0], r.rec, (float *)r.bands, r.rec);
            HIPCHK(hipGetLastError());
        }
    } else {
        hipLaunchKernelGGL(k_block_clear, dim3(nb), dim3(1), 0, c->stream, r.scal, r.rec);
        HIPCHK(hipGetLastError());
    }
    return MFB_OK;
}
// Part 2: matched filters at the picked (or fixed) shift, envelope, its spectrum, rate / phase, symbol centres, the integer stages
// of a batch, and the ONE device-to-host copy of the record(s).
static int block_enqueue_p2(mfb_ctx *c, const mfb_block_params *p, const BlkBufs &bb, uint8_t *h_dst, const BlockGeom &geo) {
    int rc;
    const int nb = bb.nb, nthreads = geo.nthreads;
    const RecPtrs r = rec_ptrs(bb);
    const size_t rec = r.rec;
    BlockScalars *scal = r.scal;
    const int *shift_dev = nullptr;
    int shift = 0;
    if (p->mode == MFB_BLOCK_SEARCH) shift_dev = &scal->shift;
    else shift = ((p->fixed_shift % c->N) + c->N) % c->N;
    if ((rc = demod_enqueue(c, bb, shift, shift_dev, (int)(rec / sizeof(int)), p->k_offset, p->k_len, p->spsym_min, geo.capacity, scal))) return rc;
    // (entries past nthreads are not part of the record: the kernel's capacity bounds what it writes; the k* == 0 fallback --
    // spSym = 10, DB:737-740, unreachable while the rate window starts above bin 0 -- is completed in block_end)
    hipLaunchKernelGGL(k_centres_block, dim3((nthreads + 255) / 256, nb), dim3(256), 0, c->stream, r.sym, r.cen, r.mag, (const cf *)bb.xc,
                       (const BlockScalars *)scal, c->N, c->M, c->W, p->op, nthreads, rec);
    HIPCHK(hipGetLastError());
    if (bb.lay.stages) {         // (batches only)
        // A12 / A13 / A14 of every block of the batch on the device (stream_kernels.hpp); the state they chain on -- the previous
        // batch's tail and bit ring -- sits in carry[cur], this batch leaves its own in carry[1 - cur]
        StreamArgs sa = c->st;
        stream_records(sa, r.d, bb.lay);
        sa.nb = nb;
        sa.nsym = nthreads;
        sa.carry_in = c->d_carry[bb.parity];
        sa.carry_out = c->d_carry[1 - bb.parity];
        hipLaunchKernelGGL(k_stream_align, dim3(nb), dim3(STREAM_ALIGN_THREADS), 0, c->stream, sa);
        HIPCHK(hipGetLastError());
        if (p->mode == MFB_BLOCK_FIXED_SHIFT && bb.clip) {
            // S-band: the clipped-peak tags in the kept trust bytes (DB:830-837), from the flight's own clip indices
            hipLaunchKernelGGL(k_stream_tag, dim3(nb, (nthreads + STREAM_TAG_THREADS - 1) / STREAM_TAG_THREADS), dim3(STREAM_TAG_THREADS), 0,
                               c->stream, sa, (const int32_t *)bb.clip->a.idx,
                               (const int32_t *)bb.clip->a.head, CLIP_HEAD);
            HIPCHK(hipGetLastError());
        }
        if (sa.K > 0) {
            int Tmax = 0;
            for (int t = 0; t < sa.K; ++t) Tmax = sa.T[t] > Tmax ? sa.T[t] : Tmax;
            stream_search_launch(c, sa, nb, Tmax);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(h_dst, r.d, rec * nb, hipMemcpyDeviceToHost, c->stream));
    return MFB_OK;
}
static int block_enqueue(mfb_ctx *c, const mfb_block_params *p, const BlkBufs &bb, uint8_t *h_dst, const BlockGeom &geo) {
    const int rc = block_enqueue_p1(c, p, bb, geo);
    return rc ? rc : block_enqueue_p2(c, p, bb, h_dst, geo);
}

// Host-to-device copy of a page-locked input buffer into its own device copy, on the input stream: it starts as soon as the
// last block that read that device copy is done -- i.e. while the block before this one is still being searched -- and the
// handle's stream picks it up with an event.  (With one device buffer and one stream the copy of an 8 MiB block, 0.15 ms,
// sat between two searches.)
// Under an integer sample format (mfb_set_sample_format) the raw bytes go to the input's staging buffer `rawslot` and k_unpack
// writes the complex64 device copy right behind the copy, on the input stream too: whatever waits for the event reads what it
// always read.  (Copy and unpack stay outside the recorded graphs, which begin behind that event.)
static int input_copy(mfb_ctx *c, const cf *src, cf *dst, size_t samples, Event *ev_h2d, Event *ev_free, int which, int rawslot) {
    if (!src || !dst) return MFB_ERR_STATE;
    if (!c->in_stream) HIPCHK(hipStreamCreateWithFlags(out(c->in_stream), hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (!ev_h2d[i]) HIPCHK(hipEventCreateWithFlags(out(ev_h2d[i]), hipEventDisableTiming));
        if (!ev_free[i]) {
            HIPCHK(hipEventCreateWithFlags(out(ev_free[i]), hipEventDisableTiming));
            HIPCHK(hipEventRecord(ev_free[i], c->stream));
        }
    }
    HIPCHK(hipStreamWaitEvent(c->in_stream, ev_free[which], 0));
    if (c->fmt != MFB_SAMPLES_CF32) {
        const int rc = raw_copy_unpack(c, src, dst, samples, rawslot, c->in_stream);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(dst, src, samples * sizeof(cf), hipMemcpyHostToDevice, c->in_stream));
    }
    HIPCHK(hipEventRecord(ev_h2d[which], c->in_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, ev_h2d[which], 0));
    return MFB_OK;
}
static int block_input_copy(mfb_ctx *c, int which) {
    return input_copy(c, which ? c->h_in2 : c->h_in, which ? c->d_x2 : c->d_x, (size_t)c->N, c->ev_h2d, c->ev_xfree, which, which);
}

// A block whose input is one of the handle's two page-locked buffers is the same sequence of launches with the same
// arguments every time (the shift the matched filters run at is read from device memory): the second such block is captured
// into a HIP graph, later ones replay it -- one call into the runtime per block instead of a dozen launches, which is what the
// host side of a stream of small blocks was spending its time on.  Any change of filters, shifts, search settings or stream
// drops the graphs (c->epoch).  MFB_NO_GRAPH=1 in the environment keeps every block on plain launches.
static bool graphs_allowed() {
    static const int off = getenv("MFB_NO_GRAPH") ? atoi(getenv("MFB_NO_GRAPH")) : 0;
    return !off;
}
static void graph_drop(BlockGraph &g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
    g.seen = false;
}
static bool same_params(const mfb_block_params &a, const mfb_block_params &b) {
    return a.mode == b.mode && a.input == b.input && a.fixed_shift == b.fixed_shift && a.k_offset == b.k_offset && a.k_len == b.k_len &&
           a.spsym_min == b.spsym_min && a.op == b.op && a.snr_window == b.snr_window && a.max_symbols == b.max_symbols &&
           a.band_capacity == b.band_capacity && a.block_stride == b.block_stride;
}

// Launch the block's (batch's) work: replay its graph, record it (second occurrence of these settings), or plain launches.
template <class Enqueue>
static int graph_or_launch(mfb_ctx *c, BlockGraph &g, const mfb_block_params *p, int nb, bool allowed, Enqueue &&enqueue) {
    int rc;
    if (allowed) {
        if (g.epoch != c->epoch || g.nb != nb || !same_params(g.params, *p)) {
            graph_drop(g);
            g.epoch = c->epoch;
            g.params = *p;
            g.nb = nb;
            g.failed = false;
        }
        if (g.exec) {
            HIPCHK(hipGraphLaunch(g.exec, c->stream));
            return MFB_OK;
        }
        if (g.seen) {
            // second block with these settings: record it (the first one went out as plain launches, so every workspace
            // it needs exists already -- nothing is allocated inside the capture)
            HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
            rc = enqueue();
            hipGraph_t graph = nullptr;
            const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
            if (rc || ce != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                (void)hipGetLastError();
                if (rc) return rc;
                g.seen = false;                       // capture not possible here: stay on plain launches
                g.failed = true;
            } else {
                hipGraphExec_t exec = nullptr;
                if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec) {
                    g.graph = graph;
                    g.exec = exec;
                    HIPCHK(hipGraphLaunch(g.exec, c->stream));
                    return MFB_OK;
                }
                (void)hipGraphDestroy(graph);
                (void)hipGetLastError();
                g.seen = false;
                g.failed = true;
            }
        } else if (!g.failed) {
            g.seen = true;
        }
    }
    return enqueue();
}

static int check_block_params(const mfb_ctx *c, const mfb_block_params *p) {
    if (!c->have_filters || (p->mode == MFB_BLOCK_SEARCH && !c->have_shifts)) return MFB_ERR_STATE;
    if (p->mode != MFB_BLOCK_SEARCH && p->mode != MFB_BLOCK_FIXED_SHIFT) return MFB_ERR_ARG;
    if (p->k_offset < 0 || p->k_len < 0 || p->k_offset + p->k_len > c->N || p->spsym_min < 2 || p->op < 0 || p->op > 2 ||
        p->max_symbols < 1 || p->snr_window < 0 || p->band_capacity < 0)
        return MFB_ERR_ARG;
    return MFB_OK;
}
// page-locked staging of a flight: at least `need` bytes (the address is baked into the slot's graphs)
static int staging_reserve(mfb_ctx *c, int slot, size_t need) {
    if (need <= c->blk_cap[slot]) return MFB_OK;
    for_each_graph(c, slot, graph_drop);
    if (c->s2) HIPCHK(hipStreamSynchronize(c->s2));
    HIPCHK(reserve(c->h_blk[slot], c->blk_cap[slot], need, need, hip_host_malloc));
    return MFB_OK;
}

static bool batch_split(const mfb_ctx *c);
static int second_stream(mfb_ctx *c, int slot);
// While one of these lives, every launch helper enqueues on the second stream (they all use c->stream) and the transforms use the
// second intermediate: part 2 of a block / batch.  The handle's stream comes back on every way out.
struct Part2Scope {
    mfb_ctx *c;
    hipStream_t s1;
    explicit Part2Scope(mfb_ctx *c_) : c(c_), s1(c_->stream) {
        c->stream = c->s2;
        c->use_z2 = true;
        c->s2_busy = true;
    }
    ~Part2Scope() {
        c->stream = s1;
        c->use_z2 = false;
    }
    Part2Scope(const Part2Scope &) = delete;
    Part2Scope &operator=(const Part2Scope &) = delete;
};
// The launches of one flight -- a block or a batch -- into slot `slot`, up to the event its _end waits for.  In one piece on the handle's
// stream (g1), or (split; second_stream has been called) part 1 there and part 2 behind it on the second stream (g2): the NEXT
// flight's part 1 is enqueued behind this one's part 1 only, and runs beside this one's part 2.  ev_free (may be null) is recorded
// behind the last reader of the input's device copy: from there on it may be overwritten.
static int flight_launch(mfb_ctx *c, BlockGraph &g1, BlockGraph &g2, const BlkBufs &bb, const mfb_block_params *p, const BlockGeom &geo,
                         int graph_nb, bool allowed, bool split, int slot, hipEvent_t ev_free) {
    int rc;
    if (!split) {
        rc = graph_or_launch(c, g1, p, graph_nb, allowed, [&]() { return block_enqueue(c, p, bb, c->h_blk[slot], geo); });
        if (rc) return rc;
        if (!bb.batch) c->have_input = true;
        HIPCHK(hipEventRecord(c->ev_blk[slot], c->stream));
        if (ev_free) HIPCHK(hipEventRecord(ev_free, c->stream));
        return MFB_OK;
    }
    rc = graph_or_launch(c, g1, p, graph_nb, allowed, [&]() { return block_enqueue_p1(c, p, bb, geo); });
    if (rc) return rc;
    if (!bb.batch) c->have_input = true;      // (the spectrum is this block's from here on, whatever becomes of part 2)
    HIPCHK(hipEventRecord(c->ev_p1[slot], c->stream));
    Part2Scope part2(c);
    if (hipStreamWaitEvent(c->stream, c->ev_p1[slot], 0) != hipSuccess) return MFB_ERR_HIP;
    rc = graph_or_launch(c, g2, p, graph_nb, allowed, [&]() { return block_enqueue_p2(c, p, bb, c->h_blk[slot], geo); });
    if (rc) return rc;
    if (hipEventRecord(c->ev_blk[slot], c->stream) != hipSuccess) return MFB_ERR_HIP;
    if (ev_free && hipEventRecord(ev_free, c->stream) != hipSuccess) return MFB_ERR_HIP;
    return MFB_OK;
}
static void flight_fill(mfb_ctx *c, BlockFlight &f, const mfb_block_params *p, const BlockGeom &geo, const RecordLayout &lay, int nb, bool clip) {
    f.active = true;
    f.mode = p->mode;
    f.nthreads = geo.nthreads;
    f.bcap = geo.bcap;
    f.shift = p->mode == MFB_BLOCK_FIXED_SHIFT ? ((p->fixed_shift % c->N) + c->N) % c->N : 0;
    f.seq = ++c->blk_seq;
    f.op = p->op;
    f.nb = nb;
    f.lay = lay;
    f.clip = clip;
    f.dsnr = c->device_snr && p->mode == MFB_BLOCK_SEARCH && geo.bcap > 0;
}
// Enqueue: everything up to and including the ONE device-to-host copy into the flight's page-locked staging; no wait.
static int block_begin(mfb_ctx *c, const mfb_block_params *p, int slot) {
    if (!c || !p || slot < 0 || slot > 1) return MFB_ERR_ARG;
    int rc = check_block_params(c, p);
    if (rc) return rc;
    if (p->input != MFB_INPUT_PINNED && p->input != MFB_INPUT_PINNED2 && p->input != MFB_INPUT_DEVICE && p->input != MFB_INPUT_UPLOADED)
        return MFB_ERR_ARG;
    if (p->input == MFB_INPUT_DEVICE && !p->device_block) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    BlockFlight &f = c->flight[slot];
    if (f.active) return MFB_ERR_STATE;          // its results have not been collected
    if (c->clip_scale > 0.f && p->input == MFB_INPUT_UPLOADED) return MFB_ERR_UNSUPPORTED;     // its samples are transformed already
    const BlockGeom geo = block_geom(c, p);
    if ((rc = blkout_reserve(c, geo.bcap > c->band_cap ? geo.bcap : c->band_cap))) return rc;
    const RecordLayout lay = rec_layout(geo.bcap, geo.nthreads);
    if ((rc = staging_reserve(c, slot, lay.bytes))) return rc;
    if (!c->ev_blk[slot]) HIPCHK(hipEventCreateWithFlags(out(c->ev_blk[slot]), hipEventDisableTiming));
    const bool pinned_in = p->input == MFB_INPUT_PINNED || p->input == MFB_INPUT_PINNED2;
    const int which = p->input == MFB_INPUT_PINNED2 ? 1 : 0;
    if (pinned_in && (rc = block_input_copy(c, which))) return rc;
    // the samples of a page-locked buffer are (being) copied by block_input_copy on the input stream; this stream waits there
    if (pinned_in) c->d_in = which ? c->d_x2 : c->d_x;
    else if (p->input == MFB_INPUT_DEVICE) c->d_in = (const cf *)p->device_block;
    // peak clip (mfb_set_peak_clip): the block's samples are clipped into the flight's buffer, which is then the block
    const bool clip = c->clip_scale > 0.f;
    ClipLaunch cl{};
    if (clip) {
        if ((rc = clip_prepare(c, slot, c->d_in, 0, 1, &cl))) return rc;
        c->d_in = c->d_clipx[slot];
    }
    const bool allowed = pinned_in && graphs_allowed() && !c->prof && !c->mirror && (p->input == MFB_INPUT_PINNED || c->h_in2);
    // two parts on two streams (mfb_set_batch_overlap), as for batches: the NEXT block's forward transform and search run beside this
    // block's matched filters, envelope transform, rate, centres and read-back.  Part 2 reads the samples (the STORE kernel), so the
    // input has to be one of the two page-locked buffers' device copies or the caller's device block -- not the handle's upload
    const bool split = batch_split(c) && p->input != MFB_INPUT_UPLOADED && c->path == MFB_PATH_SEGMENT;
    if (split) {
        if ((rc = second_stream(c, slot))) return rc;
        if (c->z2_rows < 1) {
            HIPCHK(sync_streams(c));
            HIPCHK(c->d_Z2.alloc((size_t)c->N * sizeof(cf), dev_alloc));
            c->z2_rows = 1;
        }
    }
    BlkBufs bb = single_bufs(c, lay);
    if (split && slot) bb.out = c->d_blkout2;
    if (clip) bb.clip = &cl;
    // (ev_xfree: this device copy of the input may be overwritten once the block has read it)
    rc = flight_launch(c, c->bgraph[which][slot], c->bgraph2[which][slot], bb, p, geo, split ? -1 : 0, allowed, split, slot,
                       pinned_in ? c->ev_xfree[which].get() : nullptr);
    if (rc) return rc;
    flight_fill(c, f, p, geo, lay, 0, clip);
    c->have_xc = true;
    return MFB_OK;
}

static void fill_result(mfb_block_result *r, const BlockScalars &hs, int mode, int fixed_shift) {
    r->pick[0] = hs.pick[0];
    r->pick[1] = hs.pick[1];
    r->pick_valid = hs.pick_valid;
    r->shift = mode == MFB_BLOCK_SEARCH ? hs.shift : fixed_shift;
    r->low = hs.low;
    r->high = hs.high;
    r->frac = hs.frac;
    r->cr[0] = hs.cr[0];
    r->cr[1] = hs.cr[1];
    r->cr[2] = hs.cr[2];
    r->spSym = hs.spSym;
    r->codeOffset = hs.codeOffset;
    r->count = hs.count;
    r->rate_fallback = hs.rate_fallback;
    r->band_len[0] = hs.band_len[0];
    r->band_len[1] = hs.band_len[1];
}
// One record of a collected flight to the caller: the first n symbol decisions, centres and magnitudes, the two SNR windows, the scalars
static void record_unpack(const BlockFlight &f, const uint8_t *h, const BlockScalars &hs, int n, mfb_block_result *r, int32_t *sym, int32_t *cen,
                          float *mag, float *bands_c64) {
    const RecordLayout &l = f.lay;
    memcpy(sym, h + l.sym, (size_t)n * sizeof(int));
    memcpy(cen, h + l.cen, (size_t)n * sizeof(int));
    memcpy(mag, h + l.mag, (size_t)n * sizeof(float));
    if (f.dsnr) {
        memcpy(bands_c64, h + l.bands, sizeof(cf));       // (mean_signal, mean_noise)
    } else if (f.mode == MFB_BLOCK_SEARCH && f.bcap > 0) {
        const int l0 = hs.band_len[0] < f.bcap ? hs.band_len[0] : f.bcap, l1 = hs.band_len[1] < f.bcap ? hs.band_len[1] : f.bcap;
        memcpy(bands_c64, h + l.bands, (size_t)l0 * sizeof(cf));
        memcpy(bands_c64 + (size_t)2 * f.bcap, h + l.bands + (size_t)f.bcap * sizeof(cf), (size_t)l1 * sizeof(cf));
    }
    fill_result(r, hs, f.mode, f.shift);
}

// Collect: wait for the flight's event, hand the results out.
static int block_end(mfb_ctx *c, int slot, mfb_block_result *r, int32_t *sym, int32_t *cen, float *mag, float *bands_c64) {
    if (!c || slot < 0 || slot > 1 || !r || !sym || !cen || !mag) return MFB_ERR_ARG;
    BlockFlight &f = c->flight[slot];
    if (!f.active || f.nb) return MFB_ERR_STATE;
    if (f.bcap > 0 && f.mode == MFB_BLOCK_SEARCH && !bands_c64) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_blk[slot]));
    f.active = false;
    const uint8_t *h = c->h_blk[slot];
    BlockScalars hs;
    memcpy(&hs, h + f.lay.scalars, sizeof(hs));
    int n = hs.count;
    if (n > f.nthreads) {
        // rate fallback (k* == 0 -> spSym = 10, DB:737-740; unreachable while the rate window starts above bin 0): the
        // record holds the symbols the window admits; the rest is computed now, if the matched-filter outputs are still
        // this block's
        if (c->blk_seq != f.seq) return MFB_ERR_UNSUPPORTED;
        const int nb = (n + 255) / 256;
        hipLaunchKernelGGL(k_centres, dim3(nb), dim3(256), 0, c->stream, c->d_sym, c->d_cen, c->d_mag, (const cf *)c->d_xc, hs.spSymF,
                           hs.offsetF, c->N, c->M, c->W, f.op, c->cap);
        HIPCHK(hipGetLastError());
        const int more = n - f.nthreads;
        const BackPiece bq[3] = {{sym + f.nthreads, c->d_sym + f.nthreads, (size_t)more * sizeof(int)},
                                 {cen + f.nthreads, c->d_cen + f.nthreads, (size_t)more * sizeof(int)},
                                 {mag + f.nthreads, c->d_mag + f.nthreads, (size_t)more * sizeof(float)}};
        const int rc = read_back(c, bq, 3);
        if (rc) return rc;
        n = f.nthreads;
    }
    record_unpack(f, h, hs, n, r, sym, cen, mag, bands_c64);
    return MFB_OK;
}

extern "C" int mfb_receive_block_begin(mfb_ctx *c, const mfb_block_params *p, int slot) { return block_begin(c, p, slot); }
extern "C" int mfb_receive_block_end(mfb_ctx *c, int slot, mfb_block_result *r, int32_t *sym, int32_t *cen, float *mag, float *bands_c64) {
    return block_end(c, slot, r, sym, cen, mag, bands_c64);
}
extern "C" int mfb_receive_block(mfb_ctx *c, const mfb_block_params *p, mfb_block_result *r, int32_t *sym, int32_t *cen, float *mag,
                                 float *bands_c64) {
    if (!c || !p || !r || !sym || !cen || !mag || (p->band_capacity > 0 && p->mode == MFB_BLOCK_SEARCH && !bands_c64)) return MFB_ERR_ARG;
    if (c->flight[0].active) return MFB_ERR_STATE;
    const int rc = block_begin(c, p, 0);
    if (rc) return rc;
    return block_end(c, 0, r, sym, cen, mag, bands_c64);
}

// ---- B consecutive blocks per call ---------------------------------------------------------------------------------------
// The reference's own configurations use blocks of 2^15 ... 2^17 samples with 64 bins (config/base.json:13,33): one such block
// is a few tens of microseconds of device work, and a loop that hands the device one block per turn (DP:284-338) leaves it idle
// most of the time.  Here B consecutive blocks of the stream go to the device as ONE contiguous window of
// B * stride + (N - stride) samples (stride = N - overlap: block b starts at b * stride -- the overlap between neighbours is
// shared storage, nothing is copied twice) and through ONE set of launches: batched forward FFT, one search launch over
// B x D (block, bin) streams, B picks in one launch, one matched-filter launch at the B shifts, batched envelope FFT, B rate
// estimates, the centres of all blocks, one device-to-host copy of B result records.
static int window_samples(const mfb_ctx *c, int nb) { return nb * c->win_stride + (c->N - c->win_stride); }

// the second stream of a block / batch in two parts, and the event of the flight's part 1
static int second_stream(mfb_ctx *c, int slot) {
    if (!c->s2) {
        // (the highest priority: part 2 is a latency chain whose workgroups should get the slots the big kernel frees first)
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(out(c->s2), hipStreamNonBlocking, greatest));
    }
    if (!c->ev_p1[slot]) HIPCHK(hipEventCreateWithFlags(out(c->ev_p1[slot]), hipEventDisableTiming));
    return MFB_OK;
}
// A batch on two streams (mfb_set_batch_overlap; include/mfbank.h): the handle's setting, or -- every handle -- MFB_BATCH_SPLIT=0/1 in
// the environment (the A/B switch of profiles/r06_chain.md)
static bool batch_split(const mfb_ctx *c) {
    static const int env = getenv("MFB_BATCH_SPLIT") ? atoi(getenv("MFB_BATCH_SPLIT")) : -1;
    return env >= 0 ? env != 0 : c->batch_overlap;
}
extern "C" int mfb_set_batch_overlap(mfb_ctx *c, int on) {
    if (!c || on < 0 || on > 1) return MFB_ERR_ARG;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active && c->flight[s].nb) return MFB_ERR_STATE;      // a batch is in flight
    if (c->batch_overlap != (on != 0)) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(sync_streams(c));
        ++c->epoch;               // the recorded graphs belong to the other arrangement
        c->batch_overlap = on != 0;
    }
    return MFB_OK;
}
// The two means of computeSNR's spectrum windows (DB:635-667) on the device instead of the windows themselves (snr_kernels.hpp)
extern "C" int mfb_set_device_snr(mfb_ctx *c, int on) {
    if (!c || on < 0 || on > 1) return MFB_ERR_ARG;
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    if (c->device_snr != (on != 0)) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(sync_streams(c));
        ++c->epoch;               // the recorded graphs hold the other arrangement
        c->device_snr = on != 0;
    }
    return MFB_OK;
}
extern "C" int mfb_get_block_snr(mfb_ctx *c, int slot, int block, float means[2], int32_t lens[2]) {
    if (!c || slot < 0 || slot > 1 || block < 0 || !means || !lens) return MFB_ERR_ARG;
    const BlockFlight &f = c->flight[slot];
    if (f.active || !f.dsnr || block >= (f.nb ? f.nb : 1)) return MFB_ERR_STATE;
    const uint8_t *h = c->h_blk[slot] + (size_t)block * f.lay.bytes;
    BlockScalars hs;
    memcpy(&hs, h + f.lay.scalars, sizeof(hs));
    memcpy(means, h + f.lay.bands, 2 * sizeof(float));
    lens[0] = hs.band_len[0];
    lens[1] = hs.band_len[1];
    return MFB_OK;
}
// Device buffers of the batch path, whose addresses recorded graphs hold: each group waits for what uses it and drops the graphs (epoch)
static int batch_reserve(mfb_ctx *c, int nb, size_t rec) {
    int rc;
    const size_t nbN = (size_t)nb * c->N;
    auto grow = [c](auto *cap, auto want, std::initializer_list<GrowBuf> bufs) -> int {
        HIPCHK(sync_streams(c));
        ++c->epoch;
        return grow_buffers(cap, want, bufs);
    };
    if (nb > c->bat_cap &&
        (rc = grow(&c->bat_cap, nb,
                   {{&c->d_Xb, nbN * sizeof(cf)},
                    {&c->d_xcb, nbN * c->M * sizeof(cf)},
                    {&c->d_Pb, nbN * sizeof(cf)},
                    {&c->d_envb, nbN * sizeof(float)},
                    {&c->d_sumb, (size_t)nb * c->Dtot * c->M * sizeof(float)},
                    {&c->d_resb, (size_t)nb * 2 * sizeof(float)},
                    {&c->d_crb, (size_t)nb * 3 * sizeof(float)}})))
        return rc;
    // the plain forward transforms of the batch take one row of the intermediate each
    if ((size_t)nb > c->z_rows && (rc = grow(&c->z_rows, (size_t)nb, {{&c->d_Z, nbN * sizeof(cf)}}))) return rc;
    // the two flights' records (the next batch's search writes its picks while this one's records are still read)
    if (rec * nb > c->batout_cap && (rc = grow(&c->batout_cap, rec * nb, {{&c->d_batout, rec * nb}, {&c->d_batout2, rec * nb}}))) return rc;
    // part 2's transforms (the envelopes' spectra) get an intermediate of their own
    if (batch_split(c) && (size_t)nb > c->z2_rows && (rc = grow(&c->z2_rows, (size_t)nb, {{&c->d_Z2, nbN * sizeof(cf)}}))) return rc;
    return MFB_OK;
}

static int window_buffer(mfb_ctx *c, int which, int max_blocks, int block_stride, void **host_c64) {
    if (!c || !host_c64 || which < 0 || which > 1 || max_blocks < 1 || max_blocks > 1024 || block_stride < 1 || block_stride > c->N)
        return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->win_blocks != max_blocks || c->win_stride != block_stride) {
        for (int s = 0; s < 2; ++s)
            if (c->flight[s].active && c->flight[s].nb) return MFB_ERR_STATE;      // a batch is reading the windows
        HIPCHK(sync_streams(c));
        if (c->in_stream) HIPCHK(hipStreamSynchronize(c->in_stream));
        ++c->epoch;
        for (int i = 0; i < 2; ++i) {
            c->raw_cap[2 + i] = 0;
            HIPCHK(c->h_win[i].reset());
            HIPCHK(c->d_win[i].reset());
            HIPCHK(c->d_raw[2 + i].reset());
        }
        c->win_blocks = max_blocks;
        c->win_stride = block_stride;
    }
    if (!c->h_win[which]) {
        const size_t bytes = (size_t)window_samples(c, c->win_blocks) * sizeof(cf);
        HIPCHK(c->h_win[which].alloc(bytes, hip_host_malloc));
        memset(c->h_win[which], 0, bytes);
        HIPCHK(c->d_win[which].alloc(bytes, dev_alloc));
    }
    *host_c64 = c->h_win[which];
    return MFB_OK;
}
extern "C" int mfb_window_buffer(mfb_ctx *c, int which, int max_blocks, int block_stride, float **host_c64) {
    if (c && c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the windows hold integers: mfb_window_buffer_raw
    void *p = nullptr;
    const int rc = window_buffer(c, which, max_blocks, block_stride, host_c64 ? &p : nullptr);
    if (!rc) *host_c64 = (float *)p;
    return rc;
}
extern "C" int mfb_window_buffer_raw(mfb_ctx *c, int which, int max_blocks, int block_stride, void **host, size_t *bytes) {
    if (!bytes) return MFB_ERR_ARG;
    const int rc = window_buffer(c, which, max_blocks, block_stride, host);
    if (!rc) *bytes = (size_t)window_samples(c, c->win_blocks) * (size_t)fmt_bytes(c->fmt);
    return rc;
}

extern "C" int mfb_receive_blocks_begin(mfb_ctx *c, const mfb_block_params *p, int nblocks, int slot) {
    if (!c || !p || slot < 0 || slot > 1 || nblocks < 1) return MFB_ERR_ARG;
    int rc = check_block_params(c, p);
    if (rc) return rc;
    const bool win_in = p->input == MFB_INPUT_WINDOW || p->input == MFB_INPUT_WINDOW2;
    if (!win_in && p->input != MFB_INPUT_DEVICE) return MFB_ERR_ARG;
    const int which = p->input == MFB_INPUT_WINDOW2 ? 1 : 0;
    int stride = p->block_stride;
    if (win_in) {
        if (!c->h_win[which] || nblocks > c->win_blocks) return MFB_ERR_STATE;
        if (stride == 0) stride = c->win_stride;
        if (stride != c->win_stride) return MFB_ERR_ARG;
    } else if (!p->device_block || stride < 1 || stride > c->N) {
        return MFB_ERR_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    if (c->path != MFB_PATH_SEGMENT || (p->mode == MFB_BLOCK_SEARCH && c->search_mode != MFB_SEARCH_TRANSFORMS)) return MFB_ERR_UNSUPPORTED;
    BlockFlight &f = c->flight[slot];
    if (f.active) return MFB_ERR_STATE;
    const BlockGeom geo = block_geom(c, p);
    // the stream stages' outputs go behind the core record (record_layout.hpp)
    // (fixed shift: the S-band back end; with its peak clip on, k_stream_tag adds the clipped-peak tags behind the alignment)
    const bool stages = c->st_on && nblocks <= 64;
    const RecordLayout lay = rec_layout(geo.bcap, geo.nthreads, stages);
    const size_t rec = lay.bytes;
    if ((rc = batch_reserve(c, nblocks > c->win_blocks ? nblocks : (c->win_blocks > 0 ? c->win_blocks : nblocks), rec))) return rc;
    if ((rc = staging_reserve(c, slot, rec * nblocks))) return rc;
    if (!c->ev_blk[slot]) HIPCHK(hipEventCreateWithFlags(out(c->ev_blk[slot]), hipEventDisableTiming));
    if (win_in && (rc = input_copy(c, c->h_win[which], c->d_win[which], (size_t)(nblocks * stride + (c->N - stride)), c->ev_wh2d, c->ev_wfree, which, 2 + which)))
        return rc;
    const int parity = c->carry_cur;
    // (the two flights' records live in buffers of their own: the next batch's pick writes into its records while this batch's
    // are still being read on the other stream)
    BlkBufs bb{nblocks, win_in ? (const cf *)c->d_win[which] : (const cf *)p->device_block, stride, c->d_Xb, c->d_sumb, c->d_resb, c->d_xcb,
               c->d_envb, c->d_Pb, c->d_crb, slot ? c->d_batout2 : c->d_batout, lay, true, parity, nullptr};
    // peak clip: the window's blocks are clipped into the flight's buffer (stride N), which the transforms and part 2 then read;
    // the window itself -- where neighbouring blocks share their overlap -- stays as it is
    const bool clip = c->clip_scale > 0.f;
    ClipLaunch cl{};
    if (clip) {
        if ((rc = clip_prepare(c, slot, bb.x, stride, nblocks, &cl))) return rc;
        bb.x = c->d_clipx[slot];
        bb.xstride = c->N;
        bb.clip = &cl;
    }
    const bool allowed = win_in && graphs_allowed() && !c->prof;
    mfb_block_params q = *p;
    q.block_stride = stride;
    const int gi = nblocks <= WG_NB ? nblocks : 0;
    const bool split = batch_split(c);
    if (split && (rc = second_stream(c, slot))) return rc;
    rc = flight_launch(c, c->wgraph[which][slot][parity][gi], c->wgraph2[which][slot][parity][gi], bb, &q, geo, nblocks, allowed, split, slot,
                       win_in ? c->ev_wfree[which].get() : nullptr);
    if (rc) return rc;
    if (stages) c->carry_cur = 1 - parity;        // this batch's tail and ring are the next batch's start
    flight_fill(c, f, p, geo, lay, nblocks, clip);
    c->last_batch_blocks = p->mode == MFB_BLOCK_SEARCH ? nblocks : 0;
    // the handle's one-block buffers (spectrum, matched-filter outputs) hold nothing of this batch
    c->have_xc = false;
    return MFB_OK;
}

extern "C" int mfb_receive_blocks_end(mfb_ctx *c, int slot, mfb_block_result *results, int32_t *sym, int32_t *cen, float *mag,
                                      int symbol_stride, float *bands_c64) {
    if (!c || slot < 0 || slot > 1 || !results || !sym || !cen || !mag || symbol_stride < 1) return MFB_ERR_ARG;
    BlockFlight &f = c->flight[slot];
    if (!f.active || !f.nb) return MFB_ERR_STATE;
    if (f.bcap > 0 && f.mode == MFB_BLOCK_SEARCH && !bands_c64) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_blk[slot]));
    f.active = false;
    int rc = MFB_OK;
    for (int b = 0; b < f.nb; ++b) {
        const uint8_t *h = c->h_blk[slot] + (size_t)b * f.lay.bytes;
        BlockScalars hs;
        memcpy(&hs, h + f.lay.scalars, sizeof(hs));
        int n = hs.count;
        // (the rate fallback k* == 0 -> spSym = 10 could ask for more symbols than the rate window admits; it cannot occur while
        // the window starts above bin 0, and a batch has no second pass to fetch them: the record's symbols are delivered)
        if (n > f.nthreads) {
            n = f.nthreads;
            rc = MFB_ERR_UNSUPPORTED;
        }
        if (n > symbol_stride) return MFB_ERR_ARG;
        const size_t at = (size_t)b * symbol_stride;
        record_unpack(f, h, hs, n, &results[b], sym + at, cen + at, mag + at, bands_c64 + (size_t)b * 4 * f.bcap);
    }
    return rc;
}

// What the callers of mfb_receive_blocks_end_record and mfb_debug_stream_stages learn about the records they were handed
static void fill_layout(mfb_record_layout *lay, const mfb_ctx *c, const RecordLayout &l, int nb, int symbols, int bcap, int mode, int shift) {
    memset(lay, 0, sizeof(*lay));
    lay->nblocks = nb;
    lay->record_bytes = (int64_t)l.bytes;
    lay->scalars_bytes = (int32_t)sizeof(BlockScalars);
    lay->symbols = symbols;
    lay->band_capacity = bcap;
    lay->mode = mode;
    lay->fixed_shift = shift;
    lay->off_bands = (int64_t)l.bands;
    lay->off_sym = (int64_t)l.sym;
    lay->off_cen = (int64_t)l.cen;
    lay->off_mag = (int64_t)l.mag;
    if (l.stages) {
        lay->stream_stages = 1;
        lay->off_bits = (int64_t)l.bits;
        lay->off_centres_u8 = (int64_t)l.cenw;
        lay->off_trust = (int64_t)l.trust;
        lay->off_post = (int64_t)l.post;
        lay->off_end = (int64_t)l.end;
        lay->off_hits = (int64_t)l.hits;
        lay->off_edges = (int64_t)l.edges;
        lay->edge_candidates = STREAM_EDGE_CANDS;
        lay->edge_hits = STREAM_EDGE_HITS;
        lay->max_hits = STREAM_MAX_HITS;
        lay->templates = c->st.K;
    }
}
// The whole batch as it came off the device: nb records of `rec` bytes copied into the caller's buffer, and where things are
// inside a record.  The caller (the Python host) reads scalars and arrays in place -- one copy per batch instead of a dozen
// small ones per block.
extern "C" int mfb_receive_blocks_end_record(mfb_ctx *c, int slot, void *dst, size_t capacity, mfb_record_layout *lay) {
    if (!c || slot < 0 || slot > 1 || !dst || !lay) return MFB_ERR_ARG;
    BlockFlight &f = c->flight[slot];
    if (!f.active || !f.nb) return MFB_ERR_STATE;
    const size_t rec = f.lay.bytes;
    if (capacity < rec * (size_t)f.nb) {
        // too small: say what the batch needs (nblocks * record_bytes) and leave it in flight for the caller's second attempt
        memset(lay, 0, sizeof(*lay));
        lay->nblocks = f.nb;
        lay->record_bytes = (int64_t)rec;
        return MFB_ERR_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_blk[slot]));
    f.active = false;
    memcpy(dst, c->h_blk[slot], rec * (size_t)f.nb);
    fill_layout(lay, c, f.lay, f.nb, f.nthreads, f.bcap, f.mode, f.shift);
    return MFB_OK;
}

// The integer stages behind the symbol decisions on the device, for batches (stream_kernels.hpp).
extern "C" int mfb_set_stream_stages(mfb_ctx *c, const mfb_stream_params *p) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    ++c->epoch;
    c->st_on = false;
    if (!p) return MFB_OK;                 // switched off
    // (the LUTs live in the LDS of k_stream_align: 256 rows of a bit LUT, 2048 entries of an NRZ-S LUT -- 2^xcorrMaskSize is 8 ... 32)
    if ((p->lut_mode != 1 && p->lut_mode != 2) || p->lut_rows < 1 || (p->lut_mode == 1 && p->lut_rows > STREAM_LUT8_MAX) ||
        (p->lut_mode == 2 && (p->lut_successors < 1 || (long long)p->lut_rows * 2 * p->lut_successors > STREAM_LUT3_MAX)) || !p->lut || p->overlap_samples < 2 ||
        p->overlap_samples >= c->N || p->overlap_offset < 1 || p->overlap_offset + 1 > STREAM_END_MAX || p->num_templates < 0 ||
        p->num_templates > STREAM_MAX_TMPL || (p->lut_mode == 2 && (p->lut_successors < 1 || p->lut_successors > 64)))
        return MFB_ERR_ARG;
    if (p->num_templates > 0 && (!p->templates || p->bits_overlap < 1 || p->bits_overlap > STREAM_NOV_MAX)) return MFB_ERR_ARG;
    StreamArgs &a = c->st;
    memset(&a, 0, sizeof(a));
    a.N = c->N;
    a.ovw = p->overlap_samples / 2;
    a.o = p->overlap_offset;
    a.thr = p->match_threshold;
    a.err_thr = p->error_threshold;
    a.mode = p->lut_mode;
    a.rows = p->lut_rows;
    a.succ = p->lut_mode == 2 ? p->lut_successors : 0;
    HIPCHK(c->d_lut8.reset());
    HIPCHK(c->d_lut3.reset());
    HIPCHK(c->d_sttmpl.reset());
    if (a.mode == 1) {
        HIPCHK(c->d_lut8.alloc((size_t)a.rows, dev_alloc));
        HIPCHK(hipMemcpy(c->d_lut8, p->lut, (size_t)a.rows, hipMemcpyHostToDevice));
    } else {
        const size_t n = (size_t)a.rows * 2 * a.succ * sizeof(int);
        HIPCHK(c->d_lut3.alloc(n, dev_alloc));
        HIPCHK(hipMemcpy(c->d_lut3, p->lut, n, hipMemcpyHostToDevice));
    }
    a.lut8 = c->d_lut8;
    a.lut3 = c->d_lut3;
    a.K = p->num_templates;
    a.nOv = p->bits_overlap;
    a.max_hits = STREAM_MAX_HITS;
    size_t taps = 0;
    for (int t = 0; t < a.K; ++t) {
        if (p->template_taps[t] < 1 || p->template_taps[t] > 4096) return MFB_ERR_ARG;
        a.T[t] = p->template_taps[t];
        a.thrs[t] = p->template_thresholds[t];
        a.toff[t] = (int)taps;
        taps += (size_t)a.T[t];
    }
    // the packed search (k_stream_search) takes templates of up to STREAM_PACK_TAPS taps in {-1, 0, +1}
    a.packed = a.K > 0;
    memset(a.P, 0, sizeof(a.P));
    memset(a.Q, 0, sizeof(a.Q));
    for (int t = 0; t < a.K && a.packed; ++t) {
        const int8_t *tp = p->templates + a.toff[t];
        if (a.T[t] > STREAM_PACK_TAPS) a.packed = 0;
        for (int q = 0; q < a.T[t] && a.packed; ++q) {
            const int j = a.T[t] - 1 - q;                   // window element the tap multiplies
            if (tp[q] == 1) a.P[t][j >> 5] |= 1u << (j & 31);
            else if (tp[q] == -1) a.Q[t][j >> 5] |= 1u << (j & 31);
            else if (tp[q] != 0) a.packed = 0;
        }
    }
    if (taps) {
        HIPCHK(c->d_sttmpl.alloc(taps, dev_alloc));
        HIPCHK(hipMemcpy(c->d_sttmpl, p->templates, taps, hipMemcpyHostToDevice));
    }
    a.tmpls = c->d_sttmpl;
    for (int i = 0; i < 2; ++i) {
        if (!c->d_carry[i]) HIPCHK(c->d_carry[i].alloc(sizeof(StreamCarry), dev_alloc));
        HIPCHK(hipMemset(c->d_carry[i], 0, sizeof(StreamCarry)));       // valid = 0: nothing known until mfb_stream_seed
    }
    if (!c->h_seed) HIPCHK(c->h_seed.alloc(sizeof(StreamCarry), hip_host_malloc));
    c->carry_cur = 0;
    c->st_on = true;
    return MFB_OK;
}

extern "C" int mfb_stream_seed(mfb_ctx *c, const uint8_t *post, int npost, const uint8_t *end, int nend, const uint8_t *ring, int ring_len) {
    if (!c || npost < 0 || nend < 0 || ring_len < 0 || (npost && !post) || (nend && !end) || (ring_len && !ring)) return MFB_ERR_ARG;
    if (!c->st_on) return MFB_ERR_STATE;
    if (npost > STREAM_POST_MAX || nend > STREAM_END_MAX || ring_len > STREAM_NOV_MAX) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));          // h_seed may still be on its way from the last seed
    StreamCarry *h = c->h_seed;
    memset(h, 0, sizeof(*h));
    h->valid = 1;
    h->npost = npost;
    h->nend = nend;
    if (npost) memcpy(h->post, post, (size_t)npost);
    if (nend) memcpy(h->end, end, (size_t)nend);
    h->ring_valid = ring_len > 0 && ring_len == c->st.nOv;
    h->ring_len = ring_len;
    if (ring_len) memcpy(h->ring, ring, (size_t)ring_len);
    HIPCHK(hipMemcpyAsync(c->d_carry[c->carry_cur], h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
    return MFB_OK;
}

// Test seam of the stream stages (include/mfbank.h): k_stream_align / _sync / _ring / _edges on INJECTED symbol decisions.
extern "C" int mfb_debug_stream_stages(mfb_ctx *c, int nb, int symbols, const int32_t *counts, const int32_t *sym, const int32_t *cen,
                                       const float *mag, void *dst, size_t capacity, mfb_record_layout *lay) {
    if (!c || nb < 1 || nb > 64 || symbols < 1 || !counts || !sym || !cen || !mag || !dst || !lay) return MFB_ERR_ARG;
    if (!c->st_on) return MFB_ERR_STATE;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const RecordLayout l = rec_layout(0, symbols, true);
    const size_t rec = l.bytes;
    if (capacity < rec * (size_t)nb) return MFB_ERR_ARG;
    int rc = batch_reserve(c, nb > c->bat_cap ? nb : (c->bat_cap > 0 ? c->bat_cap : nb), rec);
    if (rc) return rc;
    if (rec * nb > c->batout_cap) return MFB_ERR_ALLOC;
    std::vector<uint8_t> h(rec * (size_t)nb, 0);
    for (int b = 0; b < nb; ++b) {
        if (counts[b] < 0 || counts[b] > symbols) return MFB_ERR_ARG;
        uint8_t *r = h.data() + (size_t)b * rec;
        BlockScalars sc;
        memset(&sc, 0, sizeof(sc));
        sc.count = counts[b];
        memcpy(r + l.scalars, &sc, sizeof(sc));
        memcpy(r + l.sym, sym + (size_t)b * symbols, (size_t)symbols * sizeof(int));
        memcpy(r + l.cen, cen + (size_t)b * symbols, (size_t)symbols * sizeof(int));
        memcpy(r + l.mag, mag + (size_t)b * symbols, (size_t)symbols * sizeof(float));
    }
    HIPCHK(hipMemcpyAsync(c->d_batout, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
    StreamArgs sa = c->st;
    stream_records(sa, c->d_batout, l);
    sa.nb = nb;
    sa.nsym = symbols;
    sa.carry_in = c->d_carry[c->carry_cur];
    sa.carry_out = c->d_carry[1 - c->carry_cur];
    hipLaunchKernelGGL(k_stream_align, dim3(nb), dim3(STREAM_ALIGN_THREADS), 0, c->stream, sa);
    if (sa.K > 0) {
        int Tmax = 0;
        for (int t = 0; t < sa.K; ++t) Tmax = sa.T[t] > Tmax ? sa.T[t] : Tmax;
        stream_search_launch(c, sa, nb, Tmax);
    }
    HIPCHK(hipGetLastError());
    c->carry_cur = 1 - c->carry_cur;
    HIPCHK(hipMemcpyAsync(dst, c->d_batout, rec * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    fill_layout(lay, c, l, nb, symbols, 0, MFB_BLOCK_SEARCH, 0);
    return MFB_OK;
}

// Test seam of the one-call path (include/mfbank.h): block_pick_body / block_rate_body on injected device results.
extern "C" int mfb_debug_block_scalars(mfb_ctx *c, int n, const float *picks, const float *triples, int spsym_min, int snr_window,
                                       int max_symbols, mfb_block_result *results, float *launch_args, int32_t *band_pieces) {
    if (!c || n < 1 || !picks || !triples || !results || spsym_min < 2 || snr_window < 0 || max_symbols < 1) return MFB_ERR_ARG;
    if (!c->have_shifts) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    DevBuf<float> d_in;
    DevBuf<BlockScalars> d_out;
    std::vector<BlockScalars> h((size_t)n);
    const size_t in_bytes = (size_t)n * 5 * sizeof(float);
    if (d_in.alloc(in_bytes, hip_malloc) != hipSuccess || d_out.alloc((size_t)n * sizeof(BlockScalars), hip_malloc) != hipSuccess) return MFB_ERR_ALLOC;
    if (hipMemcpy(d_in, picks, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in + 2 * (size_t)n, triples, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return MFB_ERR_HIP;
    const int capacity = max_symbols < c->cap ? max_symbols : c->cap;
    hipLaunchKernelGGL(k_block_scalars_debug, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, (const float *)d_in,
                       (const float *)(d_in + 2 * (size_t)n), (const int *)c->d_shifts, c->Dtot, c->N, snr_window, spsym_min, capacity,
                       d_out);
    if (hipGetLastError() != hipSuccess || sync_streams(c) != hipSuccess ||
        hipMemcpy(h.data(), d_out, (size_t)n * sizeof(BlockScalars), hipMemcpyDeviceToHost) != hipSuccess)
        return MFB_ERR_HIP;
    for (int i = 0; i < n; ++i) {
        const BlockScalars &hs = h[(size_t)i];
        mfb_block_result &r = results[i];
        r.pick[0] = hs.pick[0];
        r.pick[1] = hs.pick[1];
        r.pick_valid = hs.pick_valid;
        r.shift = hs.shift;
        r.low = hs.low;
        r.high = hs.high;
        r.frac = hs.frac;
        r.cr[0] = hs.cr[0];
        r.cr[1] = hs.cr[1];
        r.cr[2] = hs.cr[2];
        r.spSym = hs.spSym;
        r.codeOffset = hs.codeOffset;
        r.count = hs.count;
        r.rate_fallback = hs.rate_fallback;
        r.band_len[0] = hs.band_len[0];
        r.band_len[1] = hs.band_len[1];
        if (launch_args) {
            launch_args[2 * i] = hs.spSymF;
            launch_args[2 * i + 1] = hs.offsetF;
        }
        if (band_pieces) memcpy(band_pieces + 8 * (size_t)i, &hs.band[0][0][0], 8 * sizeof(int32_t));
    }
    return MFB_OK;
}

static int input_buffer2(mfb_ctx *c) {
    if (!c->h_in2) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(c->h_in2.alloc((size_t)c->N * sizeof(cf), hip_host_malloc));
        memset(c->h_in2, 0, (size_t)c->N * sizeof(cf));
        if (!c->d_x2) HIPCHK(c->d_x2.alloc((size_t)c->N * sizeof(cf), dev_alloc));
    }
    return MFB_OK;
}
extern "C" int mfb_input_buffer2(mfb_ctx *c, float **p) {
    if (!c || !p) return MFB_ERR_ARG;
    if (c->fmt != MFB_SAMPLES_CF32) return MFB_ERR_STATE;      // the buffer holds integers: mfb_input_buffer_raw
    const int rc = input_buffer2(c);
    if (rc) return rc;
    *p = (float *)c->h_in2.get();
    return MFB_OK;
}
extern "C" int mfb_input_buffer_raw(mfb_ctx *c, int which, void **host, size_t *bytes) {
    if (!c || !host || !bytes || which < 0 || which > 1) return MFB_ERR_ARG;
    if (which) {
        const int rc = input_buffer2(c);
        if (rc) return rc;
    }
    *host = which ? c->h_in2 : c->h_in;
    *bytes = (size_t)c->N * (size_t)fmt_bytes(c->fmt);
    return MFB_OK;
}

extern "C" int mfb_set_sample_format(mfb_ctx *c, int format, float scale) {
    if (!c || (format != MFB_SAMPLES_CF32 && format != MFB_SAMPLES_SC16 && format != MFB_SAMPLES_SC8)) return MFB_ERR_ARG;
    float sc = 1.f;
    if (format == MFB_SAMPLES_CF32) {
        if (scale != 0.f && scale != 1.f) return MFB_ERR_ARG;      // complex64 is taken as it is
    } else if ((sc = fmt_scale_checked(format, scale)) == 0.f) {
        return MFB_ERR_ARG;
    }
    if (c->flight[0].active || c->flight[1].active) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    if (c->in_stream) HIPCHK(hipStreamSynchronize(c->in_stream));
    ++c->epoch;                  // no recorded graph outlives the element type of its input
    c->fmt = format;
    c->fmt_scale = sc;
    c->clip_restart = true;      // the chain's tail belongs to samples of the other type's stream
    // what the buffers held means nothing as the new type
    if (c->h_in) memset(c->h_in, 0, (size_t)c->N * sizeof(cf));
    if (c->h_in2) memset(c->h_in2, 0, (size_t)c->N * sizeof(cf));
    for (int i = 0; i < 2; ++i)
        if (c->h_win[i]) memset(c->h_win[i], 0, (size_t)window_samples(c, c->win_blocks) * sizeof(cf));
    return MFB_OK;
}
extern "C" int mfb_get_sample_format(mfb_ctx *c, int *format, float *scale, int *bytes_per_sample) {
    if (!c) return MFB_ERR_ARG;
    if (format) *format = c->fmt;
    if (scale) *scale = c->fmt_scale;
    if (bytes_per_sample) *bytes_per_sample = fmt_bytes(c->fmt);
    return MFB_OK;
}
// Test seam: k_unpack on nsamples host samples, the complex64 result back to the host.  The product paths do not come here.
extern "C" int mfb_debug_unpack(int device, int format, float scale, const void *raw, size_t nsamples, float *out_c64) {
    if (!raw || !out_c64 || nsamples < 1 || nsamples > ((size_t)1 << 28) || (format != MFB_SAMPLES_SC16 && format != MFB_SAMPLES_SC8))
        return MFB_ERR_ARG;
    const float sc = fmt_scale_checked(format, scale);
    if (sc == 0.f) return MFB_ERR_ARG;
    const int rc = device_ok(device);
    if (rc) return rc;
    const size_t bytes = nsamples * (size_t)fmt_bytes(format);
    DevBuf<void> d_in;
    DevBuf<cf> d_out;
    HIPCHK(d_in.alloc((bytes + 15) & ~(size_t)15, hip_malloc));
    HIPCHK(d_out.alloc(nsamples * sizeof(cf), hip_malloc));
    HIPCHK(hipMemcpy(d_in, raw, bytes, hipMemcpyHostToDevice));
    const int r = launch_unpack(format, d_in, d_out, nsamples, sc, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(out_c64, d_out, nsamples * sizeof(cf), hipMemcpyDeviceToHost));
    return MFB_OK;
}

// Test seams of the demodulation tail: k_envelope, k_code_rate / k_code_rate_block and k_centres, launched as the product launches
// them, on INJECTED inputs.  Handle-less: buffers of their own on the null stream, a synchronous copy back.
#define DBG_TAIL_MAX_ELEMS ((size_t)1 << 26)      // complex64 elements a seam takes (512 MiB)
extern "C" int mfb_debug_envelope(int device, const float *xc_c64, int nb, int M, int N, int off, float *env) {
    if (!xc_c64 || !env || nb < 1 || M < 1 || N < 1 || off < 0 || 2 * off >= M) return MFB_ERR_ARG;
    if (nb > 65535 || (size_t)nb * (size_t)M * (size_t)N > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const size_t nin = (size_t)nb * M * N, nout = (size_t)nb * N;
    DevBuf<cf> d_xc;
    DevBuf<float> d_env;
    HIPCHK(d_xc.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_env.alloc(nout * sizeof(float), hip_malloc));
    HIPCHK(hipMemcpy(d_xc, xc_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_env, 0x5a, nout * sizeof(float)));
    hipLaunchKernelGGL(k_envelope, dim3(1024, nb), dim3(256), 0, nullptr, (const cf *)d_xc, d_env, N, M, off);     // as demod_enqueue
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(env, d_env, nout * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

// k_band_means on an injected spectrum X[N] and n injected windows, one launch
extern "C" int mfb_debug_band_means(int device, const float *X_c64, int N, int n, const int32_t *pieces, float *means) {
    if (!X_c64 || !pieces || !means || N < 1 || n < 1) return MFB_ERR_ARG;
    if (n > 65535 || N > SNR_MAX_CHUNKS * SNR_CHUNK) return MFB_ERR_UNSUPPORTED;      // (the largest block: 2^22)
    for (int i = 0; i < n; ++i) {
        const int32_t *q = pieces + 4 * (size_t)i;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || (long long)q[0] + q[1] > N || (long long)q[2] + q[3] > N ||
            (long long)q[1] + q[3] > N)
            return MFB_ERR_ARG;
    }
    int rc = device_ok(device);
    if (rc) return rc;
    DevBuf<cf> d_X;
    DevBuf<int> d_p;
    DevBuf<float> d_m;
    HIPCHK(d_X.alloc((size_t)N * sizeof(cf), hip_malloc));
    HIPCHK(d_p.alloc((size_t)n * 4 * sizeof(int), hip_malloc));
    HIPCHK(d_m.alloc((size_t)n * sizeof(float), hip_malloc));
    HIPCHK(hipMemcpy(d_X, X_c64, (size_t)N * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_p, pieces, (size_t)n * 4 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_m, 0x5a, (size_t)n * sizeof(float)));
    hipLaunchKernelGGL(k_band_means, dim3(1, n), dim3(SNR_THREADS), 0, nullptr, (const float2 *)d_X.get(), (size_t)0, N, (const int *)d_p,
                       4 * sizeof(int), d_m, sizeof(float));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(means, d_m, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

#define DBG_REC_STRIDE 256       // bytes from one window's BlockScalars to the next (static_assert: sizeof(BlockScalars) <= 256)
extern "C" int mfb_debug_code_rate(int device, const float *P_c64, int nb, int n, int offset, int len, int spsym_min, int capacity,
                                   float *triples, float *block_triples, double *rate, float *launch_args, int32_t *counts) {
    if (!P_c64 || !triples || !block_triples || !rate || !launch_args || !counts || nb < 1 || n < 1) return MFB_ERR_ARG;
    if (offset < 0 || len < 0 || (long long)offset + len > n) return MFB_ERR_ARG;          // as mfb_demodulate
    if (nb > 65535 || (size_t)nb * (size_t)n > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const size_t nin = (size_t)nb * n;
    DevBuf<cf> d_P;
    DevBuf<float> d_cr;              // [2][nb][3]: k_code_rate's triples, then k_code_rate_block's
    DevBuf<uint8_t> d_sc;
    std::vector<uint8_t> recs((size_t)nb * DBG_REC_STRIDE);
    HIPCHK(d_P.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_cr.alloc((size_t)6 * nb * sizeof(float), hip_malloc));
    HIPCHK(d_sc.alloc(recs.size(), hip_malloc));
    HIPCHK(hipMemcpy(d_P, P_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_cr, 0x5a, (size_t)6 * nb * sizeof(float)));
    HIPCHK(hipMemset(d_sc, 0, recs.size()));
    for (int b = 0; b < nb; ++b)
        hipLaunchKernelGGL(k_code_rate, dim3(1), dim3(1024), 0, nullptr, (const cf *)(d_P + (size_t)b * n), d_cr + 3 * (size_t)b, offset,
                           len);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_code_rate_block, dim3(nb), dim3(1024), 0, nullptr, (const cf *)d_P, d_cr + 3 * (size_t)nb, offset, len, n,
                       spsym_min, capacity, reinterpret_cast<BlockScalars *>(d_sc.get()), (size_t)DBG_REC_STRIDE);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(triples, d_cr, (size_t)3 * nb * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(block_triples, d_cr + 3 * (size_t)nb, (size_t)3 * nb * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(recs.data(), d_sc, recs.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) {
        BlockScalars sc;
        memcpy(&sc, recs.data() + (size_t)b * DBG_REC_STRIDE, sizeof(sc));
        rate[2 * b] = sc.spSym;
        rate[2 * b + 1] = sc.codeOffset;
        launch_args[2 * b] = sc.spSymF;
        launch_args[2 * b + 1] = sc.offsetF;
        counts[2 * b] = sc.count;
        counts[2 * b + 1] = sc.rate_fallback;
    }
    return MFB_OK;
}

extern "C" int mfb_debug_centres(int device, const float *sig_c64, int M, int lenSig, int W, int op, float spSym, float offset,
                                 int capacity, int nthreads, int32_t *sym, int32_t *cen, float *mag) {
    if (!sig_c64 || !sym || !cen || !mag || M < 1 || lenSig < 1 || W < 1 || op < 0 || op > 2 || capacity < 0 || nthreads < 1)
        return MFB_ERR_ARG;
    if (!(spSym >= 2.0f) || !(offset >= 0.f) || !(offset < 2147483648.f)) return MFB_ERR_ARG;       // as mfb_find_centres; a code phase is >= 0
    if (nthreads > (1 << 20) || lenSig > (1 << 22) || (size_t)M * (size_t)lenSig > DBG_TAIL_MAX_ELEMS) return MFB_ERR_UNSUPPORTED;
    int rc = device_ok(device);
    if (rc) return rc;
    const int nblk = (nthreads + 255) / 256;
    const size_t nin = (size_t)M * lenSig, nent = (size_t)nblk * 256;
    DevBuf<cf> d_sig;
    DevBuf<int32_t> d_out;           // [3][nent]: sym, cen, mag
    HIPCHK(d_sig.alloc(nin * sizeof(cf), hip_malloc));
    HIPCHK(d_out.alloc(3 * nent * sizeof(int32_t), hip_malloc));
    HIPCHK(hipMemcpy(d_sig, sig_c64, nin * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0x5a, 3 * nent * sizeof(int32_t)));        // the canary: what the kernel leaves alone stays 0x5a5a5a5a
    hipLaunchKernelGGL(k_centres, dim3(nblk), dim3(256), 0, nullptr, (int *)d_out, (int *)(d_out + nent),
                       reinterpret_cast<float *>(d_out + 2 * nent), (const cf *)d_sig, spSym, offset, lenSig, M, W, op, capacity);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(sym, d_out, nent * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cen, d_out + nent, nent * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mag, d_out + 2 * nent, nent * sizeof(float), hipMemcpyDeviceToHost));
    return MFB_OK;
}

extern "C" int mfb_find_centres(mfb_ctx *c, float spSym, float offset, int op, int count, int32_t *sym, int32_t *cen,
                                float *mag) {
    if (!c || !sym || !cen || !mag) return MFB_ERR_ARG;
    if (!c->have_xc) return MFB_ERR_STATE;
    if (!(spSym >= 2.0f) || count < 0 || count > c->cap || op < 0 || op > 2) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    // same launch shape as the reference (ceil(N/spSym/256) blocks of 256, DB:996), bounded by capacity
    int nthreads = (int)ceil((double)c->N / (double)spSym / 256.0) * 256;
    if (nthreads > c->cap) nthreads = c->cap;
    if (nthreads < count) nthreads = count;
    const int nb = (nthreads + 255) / 256;
    // (every one of the nthreads >= count entries is written by k_centres itself: no clearing launches)
    hipLaunchKernelGGL(k_centres, dim3(nb), dim3(256), 0, c->stream, c->d_sym, c->d_cen, c->d_mag, c->d_xc, spSym, offset, c->N,
                       c->M, c->W, op, c->cap);
    HIPCHK(hipGetLastError());
    const BackPiece bp[3] = {{sym, c->d_sym, (size_t)count * sizeof(int)},
                             {cen, c->d_cen, (size_t)count * sizeof(int)},
                             {mag, c->d_mag, (size_t)count * sizeof(float)}};
    return read_back(c, bp, 3);
}

extern "C" int mfb_get_xcorr(mfb_ctx *c, float *host) {
    if (!c || !host) return MFB_ERR_ARG;
    if (!c->have_xc) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(host, c->d_xc, (size_t)c->M * c->N * sizeof(cf), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    return MFB_OK;
}

extern "C" int mfb_get_envelope(mfb_ctx *c, float *host) {
    if (!c || !host) return MFB_ERR_ARG;
    if (!c->have_xc) return MFB_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(host, c->d_env, (size_t)c->N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    return MFB_OK;
}

// ---- the side handles (stage_handle.hpp: what they share).  Each part is included here, once, where its code stood.
#include "sync_api.hpp"
#include "combine_api.hpp"
#include "mod_api.hpp"
#include "channel_api.hpp"
#include "channelize_api.hpp"
#include "synthesize_uniform_api.hpp"

// ---- N4: bit-stream alignment cross-correlation (reference lib/customXCorr.py:5-18) -----------------
// out = ifft( fft(a, N) * conj(fft(b, N)) ) with N the handle's block length: a and b are real
// sequences, truncated or zero-padded to N exactly as np.fft.fft(a, N) does.  Built from the handle's
// forward / inverse transform passes; the handle's spectrum, filter row 0 and matched-filter buffers
// serve as scratch, so this is meant for a handle of its own (M = 1), which is how the Python helper
// uses it.
__global__ void k_scale_c(cf *p, float s, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = p[i] * s;
}

extern "C" int mfb_xcorr(mfb_ctx *c, const float *a, int Na, const float *b, int Nb, float *out_c64) {
    if (!c || !a || !b || !out_c64 || Na < 1 || Nb < 1) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const int N = c->N;
    auto stage = [&](const float *src, int n) -> int {   // real sequence -> d_env, zero-padded / truncated to N
        const int k = n < N ? n : N;
        HIPCHK(hipMemcpyAsync(c->d_env, src, (size_t)k * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (k < N) HIPCHK(hipMemsetAsync(c->d_env + k, 0, (size_t)(N - k) * sizeof(float), c->stream));
        return MFB_OK;
    };
    int rc;
    if ((rc = stage(a, Na))) return rc;
    if ((rc = before_fft(c))) return rc;                                        // d_X is scratch here
    if ((rc = forward_fft(c, nullptr, c->d_env, c->d_X, 1))) return rc;        // A = fft(a, N)
    HIPCHK(sync_streams(c));                                    // d_env is reused
    if ((rc = stage(b, Nb))) return rc;
    if ((rc = forward_fft(c, nullptr, c->d_env, c->d_masks, 0))) return rc;    // conj(fft(b, N)) into filter row 0
    // inverse transform of A * conj(B): the two-pass bank kernels at shift 0, one filter row
    P1Args p1 = p1_base(c);
    p1.X = c->d_X;
    p1.shifts = nullptr;
    p1.fixed_shift = 0;
    p1.dc = 1;
    p1.M = 1;
    p1.mpb = 1;
    p1.ntiles = c->N2 / TILE;
    p1.mgroups = 1;
    p1.jsplit = 1;
    if ((rc = launch_p1<KIND_BANK>(c, p1, dim3(p1.ntiles, 1, 1)))) return rc;
    P2Args p2 = p2_base(c);
    p2_store_split(c, p2, 1);
    if ((rc = launch_p2<MODE_STORE>(c, p2, dim3(p2.parts, 1, 1)))) return rc;
    if ((rc = launch_transpose(c, c->d_xc, 1, 0))) return rc;
    hipLaunchKernelGGL(k_scale_c, dim3(256), dim3(256), 0, c->stream, c->d_xc, 1.0f / (float)N, N);   // numpy's ifft is 1/N
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_c64, c->d_xc, (size_t)N * sizeof(cf), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_streams(c));
    c->have_filters = false;   // the scratch use clobbered the bank, the spectrum and the outputs
    c->have_input = false;
    c->have_xc = false;
    return MFB_OK;
}

#ifdef MFB_SEG_TRACE
extern "C" int mfb_debug_read_trace(unsigned long long *out, int nblocks) {
    if (!out || nblocks < 1 || nblocks > 65536) return MFB_ERR_ARG;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seg_trace), (size_t)nblocks * 3 * sizeof(unsigned long long)));
    return MFB_OK;
}
#endif

extern "C" int mfb_timer_start(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return MFB_OK;
}
extern "C" int mfb_timer_stop(mfb_ctx *c, float *ms) {
    if (!c || !ms) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    HIPCHK(hipEventElapsedTime(ms, c->t0, c->t1));
    return MFB_OK;
}
extern "C" int mfb_profile_enable(mfb_ctx *c, int on) {
    if (!c) return MFB_ERR_ARG;
    c->prof = on != 0;
    return MFB_OK;
}
extern "C" int mfb_profile_read(mfb_ctx *c, int counts[2], float total_ms[2]) {
    if (!c || !counts || !total_ms) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    for (int w = 0; w < 2; ++w) {
        counts[w] = (int)(c->ev[w].size() / 2);
        double tot = 0.0;
        for (size_t i = 0; i + 1 < c->ev[w].size(); i += 2) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, c->ev[w][i], c->ev[w][i + 1]));
            tot += ms;
        }
        total_ms[w] = (float)tot;
        for (auto &e : c->ev[w]) c->ev_pool.push_back(std::move(e));
        c->ev[w].clear();
    }
    return MFB_OK;
}
extern "C" int mfb_sync(mfb_ctx *c) {
    if (!c) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_streams(c));
    return MFB_OK;
}

// ---- host copy worker (include/mfbank.h: mfb_hostcopy_*; the worker itself: hostcopy.hpp, plain C++) ----------------------------
extern "C" int mfb_hostcopy_create(mfb_hostcopy **out) {
    if (!out) return MFB_ERR_ARG;
    *out = nullptr;
    mfb_hostcopy *q = new (std::nothrow) mfb_hostcopy();
    if (!q) return MFB_ERR_ALLOC;
    if (!q->start()) {
        delete q;
        return MFB_ERR_ALLOC;
    }
    *out = q;
    return MFB_OK;
}

extern "C" int mfb_hostcopy_submit(mfb_hostcopy *q, void *dst, const void *src, size_t bytes) {
    if (!q || (bytes && (!dst || !src))) return MFB_ERR_ARG;
    if (bytes && !q->submit(dst, src, bytes)) return MFB_ERR_ALLOC;        // (no exception crosses the C ABI)
    return MFB_OK;
}

extern "C" int mfb_hostcopy_drain(mfb_hostcopy *q) {
    if (!q) return MFB_ERR_ARG;
    q->drain();
    return MFB_OK;
}

extern "C" void mfb_hostcopy_destroy(mfb_hostcopy *q) {
    if (!q) return;
    q->shutdown();
    delete q;
}
