// bank_search_api.hpp -- the Doppler search: path / basis / mode, filters, shifts, the launches of both transform paths, uploads, picks, scores.
// A part of mfbank.hip's one translation unit: included there once, behind bank_lifecycle_api.hpp and bank_input_api.hpp.  Host code only.
#pragma once

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
// Build the per-bin spectra as soon as filters, shifts and the path are known (mfb_set_filters / mfb_set_shifts / mfb_set_search_*),
// not inside the first search: 512 transforms of 2048 points for the 384-tap bank at 64 bins are 10-20 ms of host work, which does
// not belong into a receive loop's first block.  (The search still checks, and builds what is missing.)
static int fsm_prepare_eager(mfb_ctx *c) {
    if (!c->have_filters || !c->have_shifts || c->path != MFB_PATH_SEGMENT) return MFB_OK;
    const SearchPlan p = plan_search(search_inputs(c), segments(c), 1);
    return p.need_tables ? fsm_prepare(c, p) : MFB_OK;
}
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

// ---- launch helpers ------------------------------------------------------------------------------
static int fin_threads(int rows) { return 64 * (rows < 1 ? 1 : (rows > 16 ? 16 : rows)); }   // k_finalize: one wave per row
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
static int forward_fft(mfb_ctx *c, const cf *src_c, const float *src_r, cf *dst, int conj_out = 1, int rows = 1, size_t in_stride = 0) {
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

// d_in is a new block: its spectrum into d_X (and towards the host mirror); what the handle held of the block before is gone
static int new_spectrum(mfb_ctx *c) {
    int rc = before_fft(c);
    if (rc) return rc;
    rc = forward_fft(c, c->d_in, nullptr, c->d_X);
    if (rc) return rc;
    if ((rc = after_fft(c))) return rc;
    c->have_input = true;
    c->have_xc = false;
    return MFB_OK;
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
    return new_spectrum(c);
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
    return new_spectrum(c);
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
