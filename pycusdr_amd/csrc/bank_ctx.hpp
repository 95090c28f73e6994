// bank_ctx.hpp -- the bank's handle (mfb_ctx) and what every other part asks of it: waits, grow-only reserves, graph teardown, event pool, read_back.
// A part of mfbank.hip's one translation unit: included there once, first of the bank's parts.  Host code only.
#pragma once

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

// ... and no recorded graph may replay after it (epoch): what every setter and every regrow does whose change the block graphs have baked
// in.  input_too: the copies on the input stream are waited for as well (they read the page-locked inputs and the staging behind them).
static hipError_t sync_and_invalidate(mfb_ctx *c, bool input_too = false) {
    hipError_t e = sync_streams(c);
    if (e == hipSuccess && input_too && c->in_stream) e = hipStreamSynchronize(c->in_stream);
    if (e == hipSuccess) ++c->epoch;
    return e;
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
    if (c->d_part) HIPCHK(sync_and_invalidate(c));       // recorded block graphs hold the old address
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

static void graph_drop(BlockGraph &g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
    g.seen = false;
}
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
// page-locked staging of a flight: at least `need` bytes (the address is baked into the slot's graphs)
static int staging_reserve(mfb_ctx *c, int slot, size_t need) {
    if (need <= c->blk_cap[slot]) return MFB_OK;
    for_each_graph(c, slot, graph_drop);
    if (c->s2) HIPCHK(hipStreamSynchronize(c->s2));
    HIPCHK(reserve(c->h_blk[slot], c->blk_cap[slot], need, need, hip_host_malloc));
    return MFB_OK;
}

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
