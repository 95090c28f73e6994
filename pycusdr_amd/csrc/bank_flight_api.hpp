// bank_flight_api.hpp -- one flight, a block or a batch (mfb_receive_block*): the demodulation tail, its two parts, the graphs, begin and end.
// A part of mfbank.hip's one translation unit: included there once, behind the bank's search, input, clip and stream parts.  Host code only.
#pragma once

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
    // (batches only; the tags: a clipped fixed-shift batch)
    if (bb.lay.stages && (rc = stream_stages_enqueue(c, r.d, bb.lay, nb, nthreads, bb.parity, p->mode == MFB_BLOCK_FIXED_SHIFT ? bb.clip : nullptr))) return rc;
    HIPCHK(hipMemcpyAsync(h_dst, r.d, rec * nb, hipMemcpyDeviceToHost, c->stream));
    return MFB_OK;
}
static int block_enqueue(mfb_ctx *c, const mfb_block_params *p, const BlkBufs &bb, uint8_t *h_dst, const BlockGeom &geo) {
    const int rc = block_enqueue_p1(c, p, bb, geo);
    return rc ? rc : block_enqueue_p2(c, p, bb, h_dst, geo);
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

// The wait that ends a flight of either kind; the caller has checked its arguments and the slot's state, in its own order.
static hipError_t flight_wait(mfb_ctx *c, int slot) {
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipEventSynchronize(c->ev_blk[slot]);
    if (e == hipSuccess) c->flight[slot].active = false;
    return e;
}
// Collect: wait for the flight's event, hand the results out.
static int block_end(mfb_ctx *c, int slot, mfb_block_result *r, int32_t *sym, int32_t *cen, float *mag, float *bands_c64) {
    if (!c || slot < 0 || slot > 1 || !r || !sym || !cen || !mag) return MFB_ERR_ARG;
    BlockFlight &f = c->flight[slot];
    if (!f.active || f.nb) return MFB_ERR_STATE;
    if (f.bcap > 0 && f.mode == MFB_BLOCK_SEARCH && !bands_c64) return MFB_ERR_ARG;
    HIPCHK(flight_wait(c, slot));
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

extern "C" int mfb_set_batch_overlap(mfb_ctx *c, int on) {
    if (!c || on < 0 || on > 1) return MFB_ERR_ARG;
    for (int s = 0; s < 2; ++s)
        if (c->flight[s].active && c->flight[s].nb) return MFB_ERR_STATE;      // a batch is in flight
    if (c->batch_overlap != (on != 0)) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(sync_and_invalidate(c));       // the recorded graphs belong to the other arrangement
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
        HIPCHK(sync_and_invalidate(c));       // the recorded graphs hold the other arrangement
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
        HIPCHK(sync_and_invalidate(c));
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
    HIPCHK(flight_wait(c, slot));
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
    HIPCHK(flight_wait(c, slot));
    memcpy(dst, c->h_blk[slot], rec * (size_t)f.nb);
    fill_layout(lay, c, f.lay, f.nb, f.nthreads, f.bcap, f.mode, f.shift);
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
