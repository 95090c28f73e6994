/*
 * mfbank.h -- C ABI of libmfbank.so: the MI355X (gfx950) Doppler matched-filter-bank hot path.
 *
 * This is the drop-in boundary for pyCuSDR's receive hot loop.  Every entry point replaces one
 * device interaction of the reference's host driver; the citation after each prototype names the
 * reference call sites it stands in for (paths relative to pyCuSDR/ in the reference tree,
 *   DB  = demodulator/demodulator_base.py,  CU = demodulator/cuda_kernels.cu,
 *   DEC = decoder.py, CUFFT = lib/cufft.py).
 *
 * Conventions
 *   - plain C: opaque handle, raw pointers, sizes; no C++/torch types.
 *   - complex64 is passed as interleaved float pairs (re, im), exactly numpy's layout.
 *   - every function returns an int status (MFB_OK == 0); mfb_strerror() names it.  The Python
 *     wrapper raises ValueError / TypeError / MemoryError / RuntimeError from these, mirroring
 *     DB:188-190, DB:252-257, DB:306-308 and the cuFFT status table CUFFT:90-116.
 *   - ownership: the caller owns every host array it passes in; the library owns all device
 *     buffers and the pinned input buffer for the lifetime of the handle.
 *   - threading: a handle is not thread-safe; one handle per process, like the reference's one
 *     CUDA context per Demodulator_process (DB:177-181).
 *   - synchronisation: calls that return values to the host synchronise the handle's stream at
 *     the same points the reference blocks on memcpy_dtoh (DB:605, DB:730, DB:1000-1006); the
 *     *_async calls only enqueue.
 */
#ifndef MFBANK_H
#define MFBANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFB_OK               0
#define MFB_ERR_ARG          1   /* bad argument / shape      -> ValueError  (DB:188-190, 252-255) */
#define MFB_ERR_DTYPE        2   /* wrong element type        -> TypeError   (DB:256-257)          */
#define MFB_ERR_ALLOC        3   /* host/device allocation    -> MemoryError (CUFFT_ALLOC_FAILED)  */
#define MFB_ERR_HIP          4   /* HIP runtime / launch      -> RuntimeError(CUFFT_EXEC_FAILED)   */
#define MFB_ERR_STATE        5   /* filters/shifts/input unset-> RuntimeError(CUFFT_SETUP_FAILED)  */
#define MFB_ERR_UNSUPPORTED  6   /* size outside built plans  -> ValueError  (CUFFT_INVALID_SIZE)  */

typedef struct mfb_ctx mfb_ctx;

/* Operation selector of find_centres (CU:73-76, DB:31-34). */
#define MFB_CENTRES_ABS  0
#define MFB_CENTRES_REAL 1
#define MFB_CENTRES_IMAG 2

const char *mfb_strerror(int status);
/* Library/ABI version, bumped whenever a prototype changes.  No reference counterpart (its kernels are compiled from source
 * at run time, SourceModule DB:214). */
int mfb_abi_version(void);   /* 2: search paths, mfb_xcorr; 3: mfb_set_search_mode, mfb_sync_find_multi; 4: mfb_receive_block,
                              * mfb_export_rows_async, mfb_sync_find_packed; 5: mfb_debug_block_scalars; 6: mfb_receive_blocks_*,
                              * mfb_window_buffer, mfb_block_params.block_stride; 7: mfb_set_stream_stages, mfb_stream_seed,
                              * mfb_receive_blocks_end_record; 8: mfb_hostcopy_*; 9: mfb_set_batch_overlap, mfb_get_batch_scores, mfb_get_search_info, mfb_set_cu_share, mfb_receive_blocks_end_record
                              * reports the size it needs.  Calls added without a change to an existing prototype do not bump it: a caller
                              * finds them by symbol (dlsym) -- mfb_set_sample_format, mfb_get_sample_format, mfb_input_buffer_raw,
                              * mfb_window_buffer_raw, mfb_debug_unpack, mfb_debug_envelope, mfb_debug_code_rate, mfb_debug_centres, mfb_set_device_snr,
                              * mfb_get_block_snr, mfb_debug_band_means, mfb_debug_search_plan (sizeof and offsets of mfb_block_result, mfb_record_layout and
                              * BlockScalars unchanged: still 9) */

/* Create a handle on HIP device `device` for blocks of N = 2^log2N samples, `num_dopplers`
 * Doppler bins plus `doppler_offset` leading noise-reference bins (DB:150-159), M matched
 * filters, findCentres window W (odd), and the two compile-time switches the reference bakes
 * into its kernel header (SUM_ALL_MASKS, CODE_SEARCH_MASK_OFFSET; DB:398-418).
 * Replaces: cuda.Device(...).make_context() DB:177-181, buffer allocation DB:433-476,479-514,
 * FFT plan creation DB:275-338,501 and SourceModule JIT DB:214. */
int mfb_create(mfb_ctx **out, int device, int log2N, int num_dopplers, int doppler_offset,
               int M, int window_width, int sum_all_masks, int code_search_mask_offset);
/* Replaces Demodulator.__del__ (DB:517-530): frees buffers, plans, stream. */
int mfb_destroy(mfb_ctx *ctx);

/* Run all device work of this handle on an existing HIP stream (hipStream_t passed as void*),
 * e.g. torch's current stream so that RCCL collectives order naturally.  NULL restores the
 * handle's own stream.  (The reference's analogue is cufftSetStream, CUFFT:365-375.) */
int mfb_set_stream(mfb_ctx *ctx, void *hip_stream);
/* Tuning knobs (0 keeps the current value): Doppler bins per launch of the two FFT passes (bounds
 * the intermediate buffer; the reference's analogue is CUDA.batchSize, DB:301-313), matched
 * filters handled per workgroup in pass 1, FFT rows per workgroup in pass 2, and the number of
 * workgroups that share the Doppler bins of one (tile, filter group) in pass 1.  All reductions are
 * fixed-order (no float atomics), so results are bit-reproducible run to run; doppler_chunk,
 * masks_per_block and jsplit never change a result bit, rows_per_block regroups the fp32 partial
 * sums (results then agree to rounding, ~1e-7). */
int mfb_set_tuning(mfb_ctx *ctx, int doppler_chunk, int masks_per_block, int rows_per_block, int jsplit);
int mfb_get_tuning(mfb_ctx *ctx, int *doppler_chunk, int *masks_per_block, int *rows_per_block, int *jsplit);

/* Search path.  The Doppler search and the matched filtering at the chosen shift have two
 * implementations with identical results (within fp32 rounding, ~1e-7):
 *   MFB_PATH_SEGMENT  single-pass overlap-save: mfb_set_filters measures the impulse-response support
 *                     T of the bank (every shipped protocol: 48...640 taps); for T <= L/2 the block is cut
 *                     into L-point segments (L = 2^log2L, 256...8192), each mixed to the Doppler shift in
 *                     time, transformed, multiplied by the L-point filter spectra, transformed back and
 *                     reduced -- in registers and LDS, with no length-N intermediate in HBM.
 *   MFB_PATH_TWOPASS  length-N two-pass transforms through an HBM intermediate (any filter).
 * MFB_PATH_AUTO (default) takes the segment path whenever the bank allows it.  log2L = 0 chooses L by
 * a cost model; wg_per_cu (<= 64; workgroups in the grid per CU, default 32) / filters_per_pass = 0 keep the defaults.  Requesting MFB_PATH_SEGMENT for a bank
 * without short support returns MFB_ERR_UNSUPPORTED and leaves the previous setting in force.
 * (The reference's knobs of this kind are CUDA.batchSize / CUDA.streams, DB:171-178, 301-338.) */
#define MFB_PATH_AUTO    0
#define MFB_PATH_TWOPASS 1
#define MFB_PATH_SEGMENT 2
int mfb_set_search_path(mfb_ctx *ctx, int path, int log2L, int wg_per_cu, int filters_per_pass);
/* What is in force: path (TWOPASS or SEGMENT), log2L, taps T of the bank (N if it has no short
 * support), valid outputs per segment and number of segments (0 on the two-pass path).  Any pointer
 * may be NULL.  No reference counterpart (one formulation only: DB:571-591). */
int mfb_get_search_path(mfb_ctx *ctx, int *path, int *log2L, int *taps, int *valid_per_segment, int *segments);
/* Search basis (opt-in; segment path with SUM_ALL_MASKS only).  With SUM_ALL_MASKS the search needs
 * sum_m |y_m[n]|^2 only, which is invariant under any unitary mixing of the filters; the shipped banks (all 2^k
 * bit patterns of a smooth modulation) span far fewer dimensions than they have filters (GMSK 6 of 8, FSK-2 and
 * CC11xx 4 of 8, BPSK 5 of 32; directions below 1e-10 of the energy are dropped).  MFB_BASIS_SPAN makes the search transform an orthogonalised basis F of that span
 * with F F^H = C C^H (C = the taps): the same doppSum to fp32 rounding from rank(C) inverse transforms per
 * segment instead of M.  It is an algorithmic shortcut, so it is OFF by default (MFB_BASIS_FILTERS: every unique
 * filter is transformed, as the reference does, DB:578-588) and bench.py reports it as a separate figure.
 * The demodulation stage always uses the M filters.  Returns MFB_ERR_STATE on a handle created without
 * sum_all_masks (per-filter sums need every filter); on the two-pass path the request stays pending. */
#define MFB_BASIS_FILTERS 0
#define MFB_BASIS_SPAN    1
int mfb_set_search_basis(mfb_ctx *ctx, int basis);
/* Basis in force and the number of filters the search transforms per Doppler bin.  No reference counterpart (it transforms
 * all M, DB:578-588). */
int mfb_get_search_basis(mfb_ctx *ctx, int *basis, int *transformed_filters);
/* Host-only helper: dimension of the span of a bank's impulse responses (M if it has no short support).  No reference
 * counterpart: the reference transforms every length-N filter row (plans DB:292-338). */
int mfb_analyze_rank(const float *masks_c64, int M, int N, int *rank);
/* Search mode (opt-in shortcut).  The search uses only the row sums of |y|^2 over all N outputs of each circular
 * correlation (cuda_kernels.cu:421-480 after DB:578-588), and by Parseval's identity
 *     doppSum[j][m] = N/2^18 . sum_k |X[(k + shift_j) mod N]|^2 . |H_m[k]|^2
 * so MFB_SEARCH_ENERGY computes the table from the power spectrum of the block and the filters' energy spectrum
 * (their sum over m under SUM_ALL_MASKS): D.N multiply-adds, no inverse transform.  Same table to fp32 rounding, any
 * filter bank, either search path for the demodulation stage.  Because it no longer runs the matched-filter bank it
 * is OFF by default (MFB_SEARCH_TRANSFORMS) and bench.py reports it as a separate figure, never as the headline. */
#define MFB_SEARCH_TRANSFORMS 0
#define MFB_SEARCH_ENERGY     1
int mfb_set_search_mode(mfb_ctx *ctx, int mode);
int mfb_get_search_mode(mfb_ctx *ctx, int *mode);
/* Fault injection for tests: the nth device allocation made on behalf of a handle by the calling thread
 * from now on fails as if the device were out of memory (0 disarms).  Lets a test walk the free-on-error
 * path of mfb_create allocation by allocation.  nth < 0: the |nth|-th one raises std::bad_alloc inside the library instead -- what a
 * failed HOST allocation in the filter analysis or the table builders looks like; no C++ exception leaves the library: mfb_create,
 * mfb_set_filters, mfb_set_shifts, mfb_set_search_* and the mfb_analyze_* helpers return MFB_ERR_ALLOC for it, the handle (if any)
 * stays destroyable and takes a new mfb_set_filters.  No reference counterpart (teardown on error: __del__ DB:517-530). */
int mfb_debug_fail_alloc(int nth);
/* Host-only helper (no device work): common circular support window [start, start+len) of the impulse
 * responses ifft(H_m) of a filter bank complex64 [M][N]; len == N when some filter has no short support.
 * This is the analysis mfb_set_filters runs; exported so it can be checked without a GPU.  No reference counterpart: the
 * reference keeps the filters as length-N spectra only (__uploadMaskToGPU DB:246-263). */
int mfb_analyze_filters(const float *masks_c64, int M, int N, int *support_start, int *support_len);

/* Geometry the handle settled on: the two FFT factors N = N1 * N2 and, after mfb_set_filters, the number
 * of filter rows the Doppler search actually transforms (filters that are exact copies or exact
 * negatives of an earlier one are transformed once).  Any pointer may be NULL.  No reference counterpart (its cuFFT plans,
 * DB:292-338, keep their factorisation to themselves). */
int mfb_get_info(mfb_ctx *ctx, int *N1, int *N2, int *unique_filters);

/* Upload the filter bank: host complex64 [M][N], row-major, already conj(fft(template, N)) as
 * protocol.get_filter returns it.  Replaces __uploadMaskToGPU (DB:246-263).  `M`/`N` are what the
 * caller believes the shape is; a mismatch with the handle returns MFB_ERR_ARG. */
int mfb_set_filters(mfb_ctx *ctx, const float *masks_c64, int M, int N);
/* Upload the Doppler shift table int32[count] (count must equal doppler_offset + num_dopplers);
 * every entry must already be wrapped into [0, N).  Replaces memcpy_htod DB:221. */
int mfb_set_shifts(mfb_ctx *ctx, const int32_t *shifts, int count);

/* Page-locked host buffer of N complex64 owned by the handle; the caller fills it in place
 * (overlap carry included).  Replaces pagelocked_empty(...DEVICEMAP) DB:456-457 /
 * get_signalBufferHostPointer DB:1055-1060. */
int mfb_input_buffer(mfb_ctx *ctx, float **host_c64);
/* Copy the pinned buffer to the device and run the forward FFT (unnormalised, sign -1).  MFB_ERR_STATE on a handle without the
 * transforms' intermediate (an mfb_set_filters that failed while re-sizing it: set the filters again).  Replaces uploadToGPU
 * DB:548-558 (cufftExecC2C FORWARD). */
int mfb_upload(mfb_ctx *ctx);
/* Same, from an arbitrary host array of N complex64 (pageable is fine; staged through the pinned
 * buffer): the copy into the page-locked buffer that the reference's caller does itself (DB:555-556 in comments,
 * Demodulator_process DP:256,287) followed by uploadToGPU DB:548-558. */
int mfb_upload_from(mfb_ctx *ctx, const float *host_c64, int N);
/* Same, from N complex64 already resident in device memory (no copy): the forward transform of uploadToGPU DB:557-558 on a
 * caller-owned device buffer.  Used by bench.py so the timed region starts with inputs in HBM, and by the sharded path. */
int mfb_upload_device(mfb_ctx *ctx, const void *dev_c64);

/* Enqueue the Doppler search (shift-multiply, inverse FFT bank, |.|^2 row sums) for this handle's
 * bins; leaves doppSum float32 [count][M] on the device.  Replaces setArrayToZeros +
 * multInputVectorWithShiftedMasksDopp + batched cufftExecC2C INVERSE + blockAbsSumAtomic
 * (DB:571-591; CU:853-857, 339-373, 421-480). */
int mfb_search_async(mfb_ctx *ctx);
/* Copy this handle's doppSum rows into rows [row_offset, row_offset+count) of a device array
 * float32 [*][M] (e.g. the buffer that is then all-reduced across ranks).  Asynchronous.  The table is the reference's
 * GPU_bufDoppSum (filled by blockAbsSumAtomic CU:421-480, read by findDopplerEst CU:502-597); the reference never moves it. */
int mfb_export_scores_async(mfb_ctx *ctx, void *dev_dst, int row_offset);
/* Doppler pick on `dev_scores` float32 [offset+num][M] (NULL = the handle's own doppSum):
 * top-2 weighted index and metric; synchronises and returns res = {idx, metric}.
 * Replaces findDopplerEst + memcpy_dtoh (DB:601-605; CU:502-597). */
int mfb_pick(mfb_ctx *ctx, const void *dev_scores, int num, int offset, float res[2]);
/* The same two steps for the SUM_ALL_MASKS case, in which only column 0 of doppSum is populated
 * (CU:453-464): copy that column into dev_dst float32[*] at [row_offset, row_offset+count), and pick on a
 * device vector float32[offset+num] -- the sharded exchange then moves D floats instead of D*M.
 * mfb_pick_column returns MFB_ERR_STATE on a handle created without sum_all_masks. */
int mfb_export_column_async(mfb_ctx *ctx, void *dev_dst, int row_offset);
/* Row range of either form: rows [first_row, first_row + nrows) of this handle's doppSum -- whole rows of M floats
 * (column_only = 0) or column 0 alone (column_only = 1) -- to rows [dst_row, dst_row + nrows) of dev_dst.
 * Asynchronous.  With a noise-reference bin (doppler_offset > 0; DB:148-159, CU:550-554) a sharded caller moves
 * its bin slice (first_row = doppler_offset) and the replicated noise row (first_row = 0) separately. */
int mfb_export_rows_async(mfb_ctx *ctx, void *dev_dst, int dst_row, int first_row, int nrows, int column_only);
int mfb_pick_column(mfb_ctx *ctx, const void *dev_column, int num, int offset, float res[2]);
/* mfb_search_async + mfb_pick on the handle's own bins: the device part of __findUHF
 * (DB:567-605). */
int mfb_find_carrier(mfb_ctx *ctx, float res[2]);
/* Copy doppSum float32 [count][M] to the host (the reference reads it back only under
 * STORE_BITS_IN_FILE, DB:593-599); synchronises. */
int mfb_get_scores(mfb_ctx *ctx, float *host_scores);
/* Read `count` complex64 spectrum bins starting at `start` (wrapping modulo N), for the host-side
 * SNR estimate.  Replaces the zero-copy reads of GPU_bufSignalFreq_cpu_handle in computeSNR
 * (DB:651-661); synchronises. */
int mfb_get_spectrum(mfb_ctx *ctx, float *host_c64, int start, int count);

/* Matched filters at one shift + symbol-rate/phase estimate.  Runs
 *   multInputVectorWithShiftedMask (CU:174-185; DB:776-781), cufftExecC2C INVERSE batch M
 *   (DB:785), sumXCorrBuffMasks (CU:191-205; DB:717-718), cufftExecR2C (DB:721),
 *   findCodeRateAndPhase (CU:236-320; DB:725-726) over k in [k_offset, k_offset+k_len),
 * then synchronises and returns res = {k*, arg P[k*], |P[k*]|^2} (DB:730). */
int mfb_demodulate(mfb_ctx *ctx, int shift, int k_offset, int k_len, float res[3]);
/* One call per block: everything the receive loop does with a block on the device, as one stream of launches and ONE
 * synchronisation -- uploadToGPU (DB:548-558), __findUHF's search and pick (DB:567-605), its shift interpolation (DB:609-616,
 * float64, on the device), the spectrum windows computeSNR reads (DB:635-667), the matched filters at that shift, envelope,
 * R2C, findCodeRateAndPhase (DB:711-730), the float64 rate/phase arithmetic (DB:733-752), the clamp and symbol count of
 * cudaFindCentres (DB:994-999), findCentres and its three read-backs (DB:996-1006).  Results are bit-identical to the
 * sequence mfb_upload, mfb_find_carrier, mfb_get_spectrum, mfb_demodulate, mfb_find_centres with the reference's host
 * arithmetic in between (tests/test_gpu_block.py). */
enum { MFB_BLOCK_SEARCH = 0, MFB_BLOCK_FIXED_SHIFT = 1 };            /* UHF: Doppler search; STX: shift = IF offset (STX.py:21-24) */
enum { MFB_INPUT_PINNED = 0, MFB_INPUT_DEVICE = 1, MFB_INPUT_UPLOADED = 2, MFB_INPUT_PINNED2 = 3,
       MFB_INPUT_WINDOW = 4, MFB_INPUT_WINDOW2 = 5 };    /* batches: the two page-locked sample windows of mfb_window_buffer */
typedef struct mfb_block_params {
    int32_t mode;            /* MFB_BLOCK_* */
    int32_t input;           /* MFB_INPUT_PINNED(2): H2D of the (second) pinned input buffer first; _DEVICE: N complex64 at device_block;
                              * _UPLOADED: the block was uploaded by an earlier mfb_upload* call */
    const void *device_block;
    int32_t fixed_shift;     /* MFB_BLOCK_FIXED_SHIFT */
    int32_t k_offset, k_len; /* symbol-rate search window (DB:508-512) */
    int32_t spsym_min;       /* clamp of cudaFindCentres (DB:994-995) */
    int32_t op;              /* 0 |.|^2, 1 |re|, 2 |im| (DB:28-31) */
    int32_t snr_window;      /* computeSNR's windowWidth (DB:618: 5) */
    int32_t max_symbols;     /* capacity of sym / cen / mag */
    int32_t band_capacity;   /* complex64 elements per SNR window in bands_c64 [2][band_capacity]; 0 = no windows */
    int32_t block_stride;    /* mfb_receive_blocks_* only: samples from the start of a block to the start of the next (N - overlap);
                              * 0 with MFB_INPUT_WINDOW(2) = what the window was made for */
} mfb_block_params;
typedef struct mfb_block_result {
    float pick[2];           /* {index, metric} of findDopplerEst */
    int32_t pick_valid;      /* 0: NaN index, the block is to be skipped (DB:625-630); shift = 0 was demodulated */
    int32_t shift;           /* dopplerIdxlast */
    int32_t low, high;       /* int(index), ceil(index) */
    double frac;             /* index % 1 */
    float cr[3];             /* {k*, arg P[k*], |P[k*]|^2} */
    double spSym, codeOffset;/* DB:733-752 */
    int32_t count;           /* symbols written to sym / cen / mag */
    int32_t rate_fallback;   /* k* == 0: spSym = 10 (DB:737-740) */
    int32_t band_len[2];     /* elements of the signal / noise window; > band_capacity: not delivered, fetch with mfb_get_spectrum
                              * (mfb_set_device_snr: the true lengths; the windows' means are delivered instead, whatever the length) */
} mfb_block_result;
/* One block, one call: uploadAndFindCarrier (UHF.py:7-16 -> DB:548-632) + demodulate (DB:711-859, device stages). */
int mfb_receive_block(mfb_ctx *ctx, const mfb_block_params *params, mfb_block_result *result, int32_t *sym, int32_t *centres,
                      float *magnitude, float *bands_c64);
/* The same in two halves, so that the caller's sequential host stages of block i-1 (and the assembly of block i+1 in the
 * other input buffer) run while the device works on block i: _begin enqueues everything including the read-back into
 * page-locked staging and returns at once; _end waits for that block and hands its results out.  Two blocks may be in
 * flight (slot 0 / 1); they execute in the order they were begun.  mfb_input_buffer2 is the second page-locked input
 * buffer (MFB_INPUT_PINNED2).  The reference has no counterpart: its loop is strictly one block at a time (DP:284-338). */
int mfb_receive_block_begin(mfb_ctx *ctx, const mfb_block_params *params, int slot);
int mfb_receive_block_end(mfb_ctx *ctx, int slot, mfb_block_result *result, int32_t *sym, int32_t *centres, float *magnitude,
                          float *bands_c64);
int mfb_input_buffer2(mfb_ctx *ctx, float **host_c64);
/* B consecutive blocks per call.  The reference's own configurations run blocks of 2^15 ... 2^17 samples over 64 bins
 * (config/base.json:13,33; config/benchmark/bench_base.json:26; config/CC11xx.json:50) and hand the device ONE block per turn of
 * the receive loop (Demodulator_process.run, DP:284-338: popBlock, uploadAndFindCarrier, demodulate, send): a few tens of
 * microseconds of device work per turn.  These calls take `nblocks` consecutive blocks of the stream at once, as ONE contiguous
 * window of nblocks * block_stride + (N - block_stride) complex64 samples (block_stride = N - overlap; block b starts at sample
 * b * block_stride, so neighbouring blocks share their overlap samples as storage -- nothing is copied twice and the caller
 * carries the overlap once per window instead of once per block, DP:256,287,337), and run them through one set of launches:
 * batched forward FFT, ONE search launch over nblocks x bins streams, nblocks picks, ONE matched-filter launch at the nblocks
 * shifts, batched envelope FFT, rate estimates, symbol centres, ONE device-to-host copy of nblocks result records.  Every
 * number of every block equals what mfb_receive_block returns for that block alone, bit for bit (tests/test_gpu_blocks.py).
 *   mfb_window_buffer     page-locked window `which` (0 / 1) for up to max_blocks blocks (owned by the handle, zero-filled,
 *                         with a device copy of its own); asking for another geometry re-allocates both windows.
 *   _begin                params as for mfb_receive_block with input = MFB_INPUT_WINDOW / _WINDOW2 (or MFB_INPUT_DEVICE:
 *                         device_block = the window in device memory, block_stride required); enqueues and returns.  Two
 *                         batches may be in flight (slot 0 / 1, shared with mfb_receive_block_begin).  Segment search path and
 *                         MFB_SEARCH_TRANSFORMS only (else MFB_ERR_UNSUPPORTED: use the one-block calls).
 *   _end                  waits; results[nblocks]; block b's symbols / centres / magnitudes at sym + b * symbol_stride (...),
 *                         its two SNR windows at bands_c64 + b * 4 * band_capacity floats. */
int mfb_window_buffer(mfb_ctx *ctx, int which, int max_blocks, int block_stride, float **host_c64);
int mfb_receive_blocks_begin(mfb_ctx *ctx, const mfb_block_params *params, int nblocks, int slot);
/* Several demodulator instances on ONE device (the reference starts one process and one context per radio, possibly on the same
 * GPU: pyCuSDR.py:245-251, DB:177-181): give this handle's launches part `part` of `parts` equal parts of the compute units (CU i
 * belongs to part i % parts; parts = 1: the whole device again).  Without it two instances share the device without loss but not
 * evenly -- workgroups of the long-filter kernel (76 KiB of LDS) find no room beside the short-filter kernel's (52 KiB): 16 % / 85 % of
 * their stand-alone rates at BASELINE C5 --; with (0, 2) and (1, 2) each runs on its own half, whatever the other does
 * (bench.py: c5_*_shared).  The handle's own stream is re-created with a CU mask (a stream set with mfb_set_stream is the caller's
 * business); nothing may be in flight.  Known limit: the stream of the host-to-device copies carries no CU mask, so the conversion
 * of integer samples behind such a copy (mfb_set_sample_format: a few microseconds) runs outside the handle's share. */
int mfb_set_cu_share(mfb_ctx *ctx, int part, int parts);
/* How the segment search of the next block will run (no reference counterpart; bench.py's flop count reads it): filter_side = 1 when
 * the Doppler shift sits on the FILTERS' side -- the segment of samples is transformed once for `bins_per_forward` neighbouring bins
 * and every (bin, filter) brings segment spectra of its own, built from the shift table (DB:130-165) when shifts or filters change:
 * 256-point segments always, wave-local 2048-point segments for up to 8 filters and 256 MiB of spectra --, 0 when every (bin, segment)
 * is mixed in time and transformed.  Either way the table is the reference's |IFFT(X[(k + s) mod N] H_m[k])|^2 sums (CU:339-373,
 * 421-480) to fp32 rounding.  MFB_SEG_FSM=0 in the environment keeps the time-side form. */
int mfb_get_search_info(mfb_ctx *ctx, int *filter_side, int *bins_per_forward);
/* What mfb_debug_search_plan (below) is asked and answers: plain ints; a field that does not apply is 0. */
typedef struct mfb_plan_inputs {
    int32_t N, Dtot, M, MU;        /* block length, bins (num_dopplers + doppler_offset), filters, sign-unique filters */
    int32_t MB;                    /* rank of the span basis, 0 = none built */
    int32_t sum_all, uniform_mult; /* SUM_ALL_MASKS; every unique filter stands for equally many of the M */
    int32_t T;                     /* taps of the bank */
    int32_t basis_req, path_req, segl_req, seg_wpc, seg_mpb;   /* mfb_set_search_basis, mfb_set_search_path */
    int32_t num_cus;
    int32_t shifts_known;          /* a shift table of Dtot entries has been set */
    int32_t fsm, wrap_mfma;        /* MFB_SEG_FSM, MFB_SEG_WRAP_MFMA of the environment (1 = on) */
    int32_t rect_fb, rect_fs;      /* MFB_SEG_FSM_RECT (0 = automatic) */
    int32_t group;                 /* MFB_SEG_FSM_GROUP (-1 = automatic) */
} mfb_plan_inputs;
typedef struct mfb_seg_plan {      /* geometry of one k_seg launch */
    int32_t nsg, wpg, bsplit, ssplit, mpb, mgroups, igroups, grid, lds_bytes;
} mfb_seg_plan;
typedef struct mfb_search_plan {
    int32_t path, segl, V, T, Q, basis;         /* the segments: MFB_PATH_*, log2 L, valid outputs, laid-out taps, segments, MFB_BASIS_* */
    int32_t form;                               /* main launch: 0 none, 1 k_seg, 2 k_segf<256>, 3 k_segf<2048>, 4 k_segw<13, 3> */
    int32_t sumq, presum, wrap_kt;              /* k_segf's SUMQ variant, rows counted equally, K-steps of k_segw */
    int32_t pv, nfull, ntotal, parts, rows;     /* valid register slots, complete slots, slots, partial sums a row, rows a bin */
    mfb_seg_plan main_seg;                      /* form 1 */
    int32_t nsg, gbins, fb, fs, nbc, nsc, grid, lds_bytes;   /* forms 2 ... 4 */
    mfb_seg_plan tail;                          /* the masked launch over the incomplete slots (ntotal > nfull) */
    mfb_seg_plan store;                         /* the matched-filter pass of the same nblocks (mfb_demodulate, SEG_STORE) */
    int32_t need_tables, need_rows, need_span, need_segl, need_wkt;   /* the per-bin tables forms 2 ... 4 read */
} mfb_search_plan;
/* The whole plan of the next segment search of `nblocks` blocks, as the launches take it (no reference counterpart: a test seam, like
 * mfb_debug_block_scalars; csrc/search_plan.hpp).  With a handle, *inputs is FILLED from it -- what the planner is asked -- and
 * planned with the segments the handle has resolved; with ctx = NULL the given inputs are planned, segments included: host only, no
 * device and no HIP call (like mfb_analyze_rank).  MFB_ERR_UNSUPPORTED where mfb_set_search_path would refuse the inputs,
 * MFB_ERR_STATE for a handle without filters. */
int mfb_debug_search_plan(mfb_ctx *ctx_or_null, mfb_plan_inputs *inputs, int nblocks, mfb_search_plan *out);
/* The doppSum table (num_dopplers + doppler_offset rows of M floats, as mfb_get_scores: GPU_bufDoppSum, DB:594-601) of block
 * `block` of the batch begun LAST, once that batch has been collected and before the next one is begun.  MFB_ERR_STATE otherwise
 * (no batch, a fixed-shift batch, block beyond it). */
int mfb_get_batch_scores(mfb_ctx *ctx, int block, float *host_scores);
/* A batch as two parts on two streams (no reference counterpart: its loop waits for every stage of a block, DP:284-338).  Part 1 --
 * forward transforms, Doppler search, pick: the launches that fill the chip -- stays on the handle's stream; part 2 -- matched
 * filters at the picked shift, envelope, its spectrum, rate / phase, centres, the integer stages, the read-back: a chain of a dozen
 * small launches -- goes to a second stream (highest priority, transforms through an intermediate of its own, the two flights'
 * records in buffers of their own), so that the NEXT batch's part 1 runs beside this batch's part 2.  Same numbers, bit for bit
 * (the kernels and their order inside a batch do not change).  Worth +12 ... 20 % to a caller that keeps two batches in flight and is
 * not bound by its own per-block work (1.72 -> 1.92 ... 2.0 Gsamples/s at 2^15 x 64 bins x 32 blocks, 2^17 x 8: tools/batch_device_rate.py,
 * profiles/r06_chain.md); it costs a caller that waits for batch k - 1 right after it has begun batch k and is bound by its own
 * work -- the Python receive loop: -7 % -- because batch k - 1's part 2 then shares the chip with batch k's search and finishes later.
 * The one-block calls mfb_receive_block_begin / _end split the same way when it is on (input = a page-locked buffer or a device block):
 * at C2 the next block's search then runs beside this block's 0.16 ms of demodulation stage, 1.578 -> 1.518 ms per block with two
 * blocks in flight (tools/block_device_rate.py).  Off by default (0); the environment's MFB_BATCH_SPLIT=0/1 overrides every handle. */
int mfb_set_batch_overlap(mfb_ctx *ctx, int on);
int mfb_receive_blocks_end(mfb_ctx *ctx, int slot, mfb_block_result *results, int32_t *sym, int32_t *centres, float *magnitude,
                           int symbol_stride, float *bands_c64);
/* The integer stages behind the symbol decisions, on the device, for the blocks of a batch (mfb_receive_blocks_*; UHF search
 * mode and S-band fixed-shift mode alike).  Replaces, block by block and bit for bit:
 *   A12  extractBits (DB:1012-1023: bits = bitLUT[sym]) -- lut_mode 1, lut = uint8[lut_rows] of 0 / 1 -- or extractBitsNRZs
 *        (DB:1026-1051) -- lut_mode 2, lut = int32[lut_rows][2][lut_successors] = symbolLUT[sym][is-one | is-zero][successors],
 *        impossible transitions -> 0 and counted (lut_rows <= 256 resp. lut_rows * 2 * lut_successors <= 2048: MFB_ERR_ARG beyond);
 *   A13  checkSymbolOverlap (DB:863-988): the symbols whose centre lies in [overlap_samples / 2, N - overlap_samples / 2], the
 *        +-1 repair against the previous block over overlap_offset symbols with match_threshold (DB:97-99, 938-957), skipped
 *        above error_threshold impossible transitions (DB:925), and the uint8 casts of DB:859 (centres mod 256; trust = the raw
 *        bytes of the leading fp32 magnitudes, DB:472,1005-1006);
 *   A14  the decoder's two searches np.where(np.convolve(stream, template) >= threshold) (DEC:96-113) on the stream it stitches
 *        when no candidate is stashed -- the last bits_overlap bits before the block + the block's bits (DEC:89-90) -- for up to
 *        two templates of taps in {-1, 0, +1} (header mask, sync flag), thresholds numOnes - tolerance (DEC:101,113).
 * A block whose case is irregular (a symbol index outside the LUT, no first / last centre, a window or a previous tail too
 * short for the slices numpy would take) is flagged (a13_status 0) and left to the host path, which does whatever the
 * reference does there; the sync hits are flagged invalid from such a block to the end of the batch (and until the caller
 * seeds the state again).  The state a batch starts from -- the previous block's tail (bits behind its window: poswinP, last
 * overlap_offset + 1 bits inside it: posSymEnd, DB:977-979) and the last bits_overlap bits of the stream -- stays on the device
 * from batch to batch; mfb_stream_seed sets it from the host's (start of a stream, after an irregular block, after blocks
 * that went another way).  Batches of more than 64 blocks run without the stages (their records carry layout.stream_stages = 0: the
 * host does A12 ... A14 for them): one workgroup chains the kept-bit counts of a batch's blocks through one wave, 64 lanes.
 * Batches at a FIXED shift (MFB_BLOCK_FIXED_SHIFT, the S-band back end demodulator/STX.py:8-24) run the same stages under the
 * same conditions.  That back end also tags the symbols next to clipped interference peaks in the trust bytes (DB:830-837): with
 * the peak clip on (mfb_set_peak_clip), a kernel behind A13 sets the kept trust byte of every symbol whose full centre c has a
 * clipped-sample index p of its block with lo(p) <= c < hi(p) -- s = ceil(spSym) of the record (float64, unclamped), hi(p) =
 * min(p + 2 s + 1, N), lo(p) = p - 2 s, or max(p - 2 s + N, 0) when that is negative: numpy's slice marks[p - 2s : p + 2s + 1] --
 * to 254 (int8 -2), from the flight's own clip indices; the record's scalars say so (BlockScalars.clip_tag = 1, clip_count = the
 * block's number of indices).  Those two fields are written only in such batches (fixed shift, stages, peak clip on): in any
 * other record they hold whatever an earlier flight left there and mean nothing.  Without the peak clip there is nothing to tag.  An irregular block (a13_status 0) is tagged by
 * the host with the rest of its stages.  p == NULL switches the stages off. */
typedef struct mfb_stream_params {
    int32_t overlap_samples;     /* 2^overlap (config GPU.overlap) */
    int32_t overlap_offset;      /* symbol_check_overlap_offset (DB:19-26): 20 */
    int32_t match_threshold;     /* overlap_offset - symbol_check_match_num_errors_allowed */
    int32_t error_threshold;     /* symbol_check_error_threshold */
    int32_t lut_mode, lut_rows, lut_successors;
    const void *lut;
    int32_t num_templates;       /* 0: no sync search */
    int32_t bits_overlap;        /* protocol.numBitsOverlap */
    int32_t template_taps[2], template_thresholds[2];
    const int8_t *templates;     /* taps back to back, as np.convolve takes them (the flipped +-1 masks) */
} mfb_stream_params;
/* A12 / A13 / A14 on the device (DB:1012-1051, DB:863-988, DEC:89-113: the block comment above); mfb_stream_seed hands over what
 * the host keeps between blocks: poswinP / posSymEnd (DB:977-979) and the tail of bitsOverlapBuf (DEC:90). */
int mfb_set_stream_stages(mfb_ctx *ctx, const mfb_stream_params *params);
int mfb_stream_seed(mfb_ctx *ctx, const uint8_t *post, int npost, const uint8_t *end, int nend, const uint8_t *ring, int ring_len);
/* A finished batch as it came off the device: nblocks records of record_bytes each copied into dst (capacity bytes), and where
 * things are inside a record -- the scalars (struct BlockScalars of csrc/small_kernels.hpp, scalars_bytes long, at offset 0),
 * the two SNR windows, int32 symbols / centres and float32 magnitudes (`symbols` entries each; `count` of them valid), and
 * with the stream stages on: kept bits / centres mod 256 / trust bytes (uint8, a13_nwin valid), the block's tail (post: a13_npost
 * bytes, end: a13_nend), the sync hits (per template: int32 idx[max_hits] | score[max_hits]; sync_count valid).  One copy per
 * batch instead of one call per array and block: what mfb_receive_blocks_end hands out, read in place (DB:1000-1006 reads
 * three arrays per block with three memcpy_dtoh).  capacity < nblocks * record_bytes: MFB_ERR_ARG with layout->nblocks and
 * layout->record_bytes filled in (everything else zero) and the batch STILL in flight -- call again with a buffer of that size. */
typedef struct mfb_record_layout {
    int32_t nblocks, scalars_bytes, symbols, band_capacity, mode, fixed_shift, stream_stages, max_hits, templates, reserved;
    int32_t edge_candidates, edge_hits;   /* per block: the leading T - 1 positions of the stream a FIXED-mode decoder would restart
                                           * at for each of the first header hits (DEC:254-263): int32 {a_rel, valid, n[2],
                                           * idx[2][edge_hits], score[2][edge_hits]} each, at off_edges */
    int64_t record_bytes, off_bands, off_sym, off_cen, off_mag, off_bits, off_centres_u8, off_trust, off_post, off_end, off_hits,
            off_edges;
} mfb_record_layout;
int mfb_receive_blocks_end_record(mfb_ctx *ctx, int slot, void *dst, size_t capacity, mfb_record_layout *layout);
/* Test seam of the stream stages: the same kernels on INJECTED symbol decisions -- counts[nb], and per block `symbols` entries of
 * symbol index / centre / magnitude, as findCentres writes them (DB:996-1006) -- in front of the state the last mfb_stream_seed (or
 * batch) left; the records come back as mfb_receive_blocks_end_record delivers them.  Lets a test drive the alignment through
 * planted +-1 slips, impossible transitions and irregular blocks and compare with the host's checkSymbolOverlap / extractBits*
 * (DB:863-1051) bit for bit (tests/test_gpu_stream_stages.py).  Advances the device-side state like a batch. */
int mfb_debug_stream_stages(mfb_ctx *ctx, int nb, int symbols, const int32_t *counts, const int32_t *sym, const int32_t *centres,
                            const float *magnitude, void *dst, size_t capacity, mfb_record_layout *layout);
/* Test seam of the one-call path.  mfb_receive_block moved two pieces of the reference's float64 HOST arithmetic onto the
 * device: the shift interpolation and the bounds of computeSNR's spectrum windows behind the pick (DB:609-620, 635-667), and
 * samples per symbol / code phase / clamp / symbol count behind the rate argmax (DB:733-752, 994-999).  This call runs exactly
 * those two device stages (the same device functions, one thread per item) on n INJECTED device results instead of the ones
 * the search and the argmax produced -- picks float[n][2] = {index, metric} as findDopplerEst writes them, triples float[n][3]
 * = {k*, arg P[k*], |P[k*]|^2} as findCodeRateAndPhase writes them -- with the handle's shift table and block length.  That is
 * the point at which the reference's own code can be fed the same values (a recording fake of its memcpy_dtoh,
 * tests/golden/make_golden_host.py), so reference-run fixtures gate this arithmetic bit for bit (tests/test_gpu_pins_host.py).
 * results[n]: as mfb_receive_block fills them (no symbols are decided); launch_args float[n][2] (optional): the two float32
 * values findCentres is launched with (DB:997); band_pieces int32[n][2][2][2] (optional): [signal | noise][piece][start, length]
 * of the spectrum windows.  No effect on the handle's state. */
int mfb_debug_block_scalars(mfb_ctx *ctx, int n, const float *picks, const float *triples, int spsym_min, int snr_window,
                            int max_symbols, mfb_block_result *results, float *launch_args, int32_t *band_pieces);

/* Interference-peak clipping on the device, in front of the forward transform of mfb_receive_block(_begin) and
 * mfb_receive_blocks_begin -- the reference's __thresholdInput (DB:670-707), which the S-band back end runs on every block on the
 * host.  Twice: |x| of every sample, t = (float)scale * mean|x|, every sample above t scaled to magnitude t; |x| of the clipped
 * samples again, a second threshold, a second clip.  The clipped samples and the ascending indices of the second round
 * (clippedPeakIPure) equal numpy's on the host bit for bit -- its |x| (max * sqrt(fma(r, r, 1)), r = min / max), its pairwise
 * float32 mean over 8192-element chunks, its complex arithmetic -- for blocks of N = 2^k >= 4096 samples (smaller handles:
 * MFB_ERR_UNSUPPORTED).  The clipped block goes to a buffer of the flight (the caller's samples and windows stay as they are),
 * which the transforms and the matched filters then read.
 *   scale      0 switches clipping off (the default), > 0 is the reference's peakThresholdScale.
 *   overlap    > 0: chain consecutive blocks as the reference's loop does (it carries the overlap AFTER clipping,
 *              DP:293,337): a block's first `overlap` samples are replaced by the previous block's clipped last `overlap`
 *              samples -- inside a batch and from call to call; 0: every block is clipped as given.
 * Every call restarts the chain; MFB_INPUT_UPLOADED with clipping on returns MFB_ERR_UNSUPPORTED.  Nothing may be in flight. */
int mfb_set_peak_clip(mfb_ctx *ctx, float scale, int overlap);
/* The next block's overlap is taken as given (the previous block did not go through the device clip; DB:670-707). */
int mfb_restart_peak_clip(mfb_ctx *ctx);
/* The chain's tail (DB:670-707): the last device-clipped block's clipped last `overlap` samples (count must equal the overlap of
 * mfb_set_peak_clip), *valid = 0 when there is none (clipping off, no overlap, chain restarted).  For a caller that goes on with
 * the host's clip after device-clipped blocks: the reference carries the overlap after clipping (DP:293,337).  Synchronises;
 * nothing may be in flight. */
int mfb_get_peak_clip_tail(mfb_ctx *ctx, float *host_c64, int count, int32_t *valid);
/* clippedPeakIPure (DB:670-707) of block `block` (0 for mfb_receive_block_*) of the flight collected last from `slot`: *count =
 * the number of indices, the first min(count, cap) of them (ascending) into idx.  Valid until `slot` is begun again (each slot keeps its own buffers).
 * MFB_ERR_STATE if that flight is not collected or was not clipped. */
int mfb_get_block_clips(mfb_ctx *ctx, int slot, int block, int32_t *idx, int cap, int32_t *count);

/* computeSNR's two means on the device (DB:635-667).  The reference takes 20 log10(mean|X_sig| / mean|X_noise| - 1) over two windows
 * of the block's spectrum on the host (DB:651-661); the block calls above deliver those windows up to band_capacity elements, and a
 * block of a batch whose windows are longer has no SNR.  With this mode on (off by default), every SEARCHED block of
 * mfb_receive_block, mfb_receive_block_begin / _end, mfb_receive_blocks_begin / _end and _end_record gets a launch behind its pick that
 * computes np.mean(np.abs(window)) of both windows as float32 -- window = piece 0 then piece 1 of BlockScalars.band, np.concatenate's
 * order when the band wraps around 0 Hz; numpy's |x|, its pairwise float32 sum over 8192-element chunks, (float)((double)sum / n); NaN
 * for an empty window -- bit for bit what numpy gives from the spectrum slices, for windows of ANY length (csrc/snr_kernels.hpp).
 * Delivery: the first complex64 element of the block's signal-window region -- in its record (off_bands) and in bands_c64 (block b:
 * bands_c64 + b * 4 * band_capacity floats) -- is (mean_signal, mean_noise); NO spectrum sample is copied, so band_capacity may be 1;
 * band_len still reports the windows' true lengths; the device-to-host copy stays one per flight.  With the mode on and
 * band_capacity == 0 the record has no room for them: the means are NOT computed and NOT delivered.  Fixed-shift blocks have no pick
 * and no SNR, as before.  With the mode off nothing changes: no launch, no byte of any record.
 * Switching drops the recorded graphs; MFB_ERR_STATE while anything is in flight. */
int mfb_set_device_snr(mfb_ctx *ctx, int on);
/* The same two means (DB:651-661: np.mean(np.abs(...)) of the signal and of the noise window) and the windows' lengths of block
 * `block` (0 for mfb_receive_block_*) of the flight collected last from `slot`.  Valid until `slot` is begun again.  MFB_ERR_STATE if
 * that flight is not collected, was not searched with mfb_set_device_snr on, or had band_capacity == 0. */
int mfb_get_block_snr(mfb_ctx *ctx, int slot, int block, float means[2], int32_t lens[2]);
/* Test seam of mfb_set_device_snr: the same kernel and device function (DB:651-661 on the device) on an INJECTED spectrum X_c64
 * complex64 [N] and n injected windows pieces int32 [n][2][2] = [piece][start, length], in one launch; means float32 [n].
 * MFB_ERR_ARG for a piece outside [0, N] or a window longer than N.  Handle-less, on `device`. */
int mfb_debug_band_means(int device, const float *X_c64, int N, int n, const int32_t *pieces, float *means);

/* Symbol centres on the matched-filter outputs left by mfb_demodulate.  Replaces findCentres
 * (CU:78-146) + the three memcpy_dtoh of cudaFindCentres (DB:996-1006).  Writes `count` =
 * int(N/spSym) entries (must be <= capacity) of symbol index, centre sample and fp32 magnitude. */
int mfb_find_centres(mfb_ctx *ctx, float spSym, float offset, int op, int count,
                     int32_t *host_sym, int32_t *host_centre, float *host_mag);
/* Copy the matched-filter outputs complex64 [M][N] to the host (debug/parity; the reference does
 * this only under STORE_BITS_IN_FILE, DB:849-850). */
int mfb_get_xcorr(mfb_ctx *ctx, float *host_c64);
/* Copy the symbol-energy envelope float32 [N] (output of sumXCorrBuffMasks, CU:191-205; launched at DB:717-718) to the host. */
int mfb_get_envelope(mfb_ctx *ctx, float *host_f32);

/* Batched sync/preamble correlation: for each of B bit streams (uint8 0/1, length L, row-major
 * [B][L]) the full convolution with an integer template int8[T]:
 *   score[b][i] = sum_t tmpl[t] * bits[b][i - t],   i in [0, L+T-1)
 * exactly what np.convolve(bits, tmpl) returns at DEC:96 and DEC:112, as int32 [B][L+T-1].
 * Host pointers in, host pointer out; runs on `device`. */
int mfb_sync_correlate(int device, const uint8_t *bits, int B, int L,
                       const int8_t *tmpl, int T, int32_t *scores);

/* Thresholded form of the same correlation: for every stream the positions i (ascending) with
 * score[b][i] >= threshold and their scores -- exactly np.where(np.convolve(bits, tmpl) >= threshold)
 * as used at DEC:101 and DEC:113 -- without moving the full score arrays to the host.
 * counts[b] receives the TOTAL number of hits of stream b; the first min(counts[b], max_hits) of them
 * are stored in hit_idx[b][..] / hit_score[b][..] (row stride max_hits).  A caller that sees
 * counts[b] > max_hits repeats the call with a larger max_hits (or uses mfb_sync_correlate). */
int mfb_sync_find(int device, const uint8_t *bits, int B, int L, const int8_t *tmpl, int T,
                  int threshold, int max_hits, int32_t *hit_idx, int32_t *hit_score, int32_t *counts);

/* The same for several templates in one call: the decoder correlates every block's bit stream with the header mask
 * AND the sync flag (DEC:96-101 and DEC:112-113).  Template t has T[t] taps at tmpls + T[0] + ... + T[t-1] and threshold
 * thresholds[t]; its results are counts[t*B + b], hit_idx / hit_score[(t*B + b)*max_hits + ..].  ntmpl <= 16.  Small
 * calls (<= 1 MiB of bits and of results) move inputs and results as one packed copy each through page-locked
 * staging: one host-device round trip per block instead of two calls x five copies. */
int mfb_sync_find_multi(int device, const uint8_t *bits, int B, int L, const int8_t *tmpls, const int *T,
                        const int *thresholds, int ntmpl, int max_hits, int32_t *hit_idx, int32_t *hit_score,
                        int32_t *counts);

/* A decoder's own sync finder: the templates and thresholds it searches in every block's bit stream (header mask and sync flag,
 * DEC:96-113) stay on the device with a stream (highest priority), page-locked staging and result buffers of the finder's own.
 * _begin copies the stream in, enqueues the search and returns at once; _end waits and hands out, per template t,
 * counts[t] and the first min(counts[t], max_hits) positions / scores at hit_idx + t*max_hits (ascending).  One search in
 * flight per finder.  The reference computes both correlations with np.convolve on the host, synchronously. */
typedef struct mfb_syncfinder mfb_syncfinder;
int mfb_syncfinder_create(mfb_syncfinder **out, int device, const int8_t *tmpls, const int *T, const int *thresholds, int ntmpl,
                          int max_bits, int max_hits);
int mfb_syncfinder_destroy(mfb_syncfinder *finder);
int mfb_syncfinder_begin(mfb_syncfinder *finder, const uint8_t *bits, int L);
int mfb_syncfinder_end(mfb_syncfinder *finder, int32_t *counts, int32_t *hit_idx, int32_t *hit_score);

/* The same search on PACKED bit streams -- 8 bits per byte in numpy.packbits layout (stream bit i = bit 7 - i%8 of byte
 * i/8), row b at packed + b*row_bytes -- for taps in {-1, 0, +1}: the correlation is popcount(W & P) - popcount(W & Q) on
 * 64-bit windows (exact), an eighth of the bytes cross the host link, and only the hits come back, as ONE flat list: stream
 * b's hits (ascending position) start at sum(counts[0..b)).  total_hits may exceed max_total: the lists then hold the
 * first max_total hits, call again with more room.  device_ms (optional): kernel time between the copies, from HIP
 * events.  Returns MFB_ERR_UNSUPPORTED for other tap values.  Replaces np.convolve + np.where of DEC:96-113 for batches.
 * mfb_sync_pinned_buffer: a page-locked buffer of at least `bytes` owned by the library (per device) that a caller may
 * produce its packed streams into, so that their copy to the device is a plain asynchronous DMA. */
int mfb_sync_find_packed(int device, const uint8_t *packed_bits, int B, int L, int row_bytes, const int8_t *tmpl, int T,
                         int threshold, int max_total, int32_t *hit_idx, int32_t *hit_score, int32_t *counts,
                         int32_t *total_hits, float *device_ms);
int mfb_sync_pinned_buffer(int device, size_t bytes, void **host);

/* Bit-stream alignment cross-correlation of the soft combiner:
 *   out = ifft( fft(a, N) * conj(fft(b, N)) ),  N = the handle's block length,
 * a, b real float32 sequences truncated / zero-padded to N as np.fft.fft(a, N) does; out complex64 [N].
 * Replaces customXCorr (lib/customXCorr.py:5-18; call site softCombiner.py:701-706).  Uses the handle's
 * spectrum / filter / output buffers as scratch: give it a handle of its own (M = 1); filters and input
 * of the handle are invalidated. */
int mfb_xcorr(mfb_ctx *ctx, const float *a, int Na, const float *b, int Nb, float *out_c64);

/* The soft combiner's deterministic core on the device: softCombiner.py:665-798 (correlate), softCombiner.py:570-618 (_doVoteN),
 * softCombiner.py:623-662 (_doVote2).  The master's new bits bM[Lm] (uint8 0/1) and trust tM[Lm] (int8) are aligned against every
 * slave's whole buffer bT_i[n_i], tT_i[n_i], in the caller's order.  The current master length Lc starts at Lm; per slave, with
 * N = 2^ceil(log2 n):
 *   x[k] = sum_{j < min(Lc, n)} bT[(j + k) mod N] * bM[j],  k in [0, N), bT zero beyond n
 *          -- abs(customXCorr(bitsX, bitsM[:n])) of softCombiner.py:706 as exact integers (popcounts of packed words);
 *   val[0..14], idx0: the fifteen largest x by repeated arg-max with zeroing, ties to the lowest index (softCombiner.py:713-716);
 *   cond = mean(val[2:]) + variance_multiplier * std(val[2:]) in float64; the slave is matched when val[0] > cond;
 *   a matched slave contributes bT[idx0 : idx0 + Lc]; avail = max(0, min(Lc, n - idx0)) is what that slice holds.  avail <
 *   min_length: the whole call yields nothing (the reference's `return None`, softCombiner.py:733-737); avail < Lc: Lc = avail for
 *   the master and every slave accepted before (softCombiner.py:738-747), and the next slave is correlated with the shortened master.
 * K matched slaves: K >= 2 vote with _doVoteN, K = 1 with _doVote2 -- both through the tables of mfb_combiner_set_vote --, K = 0
 * passes the master's bits and trust through.  Deviation: a slave of n < 16 bits is not evaluated and not matched (the reference
 * would raise or match noise on such a buffer).  The counter / length rule by which the reference holds back an unmatched master
 * (softCombiner.py:779-786) is bookkeeping of the caller, not part of this core.
 * Limits: at most MFB_COMBINE_MAX_SLAVES slaves (four voters) and streams of at most 2^20 bits; MFB_ERR_UNSUPPORTED beyond, and the
 * caller takes its host path. */
#define MFB_COMBINE_MAX_SLAVES 3
#define MFB_COMBINE_NOTHING     0   /* a matched slave overlaps by less than min_length: no output */
#define MFB_COMBINE_COMBINED    1   /* voted with matched_count >= 1 slaves */
#define MFB_COMBINE_MASTER_ONLY 2   /* no slave matched: the master's bits and trust, unchanged */
typedef struct mfb_combine_params {
    double variance_multiplier;                 /* conf['SoftCombiner']['varianceMultiplier'] */
    int32_t min_length;                         /* conf['SoftCombiner']['minProcessingLength'] */
    int32_t master_len;                         /* Lm */
    int32_t num_slaves;
    int32_t slave_len[MFB_COMBINE_MAX_SLAVES];  /* n_i */
} mfb_combine_params;
typedef struct mfb_combine_slave {
    int32_t evaluated;      /* 0: n < 16, or the call had already ended in MFB_COMBINE_NOTHING; everything else is 0 then */
    int32_t matched;
    int32_t idx0;           /* lag of val[0] */
    int32_t avail;          /* matched slaves only */
    int32_t lc_after;       /* Lc after this slave */
    int32_t reserved;
    int32_t val[15];
    int32_t reserved2;
    double cond;
} mfb_combine_slave;
typedef struct mfb_combine_result {
    int32_t status;         /* MFB_COMBINE_* */
    int32_t out_len;        /* bits and trust bytes handed out; 0 for MFB_COMBINE_NOTHING */
    int32_t matched_count;
    int32_t num_slaves;
    int32_t matched_slaves[MFB_COMBINE_MAX_SLAVES];   /* indices into the call's slave list, in the caller's order */
    int32_t reserved;
    mfb_combine_slave slave[MFB_COMBINE_MAX_SLAVES];
} mfb_combine_result;
/* A combiner owns a stream, page-locked staging and device buffers for streams of up to max_bits bits and max_slaves slaves
 * (shaped like mfb_syncfinder_*).  The reference keeps these arrays in numpy (Worker.data, softCombiner.py:137-147). */
typedef struct mfb_combiner mfb_combiner;
int mfb_combiner_create(mfb_combiner **out, int device, int max_bits, int max_slaves);
int mfb_combiner_destroy(mfb_combiner *c);
/* The vote tables for `voters` = 2, 3 or 4 (master + matched slaves): entries = 8^voters; entry sum_v code_v * 8^v with
 * code_v = 4 * bit_v + trust class {< -1: 0, -1: 1, 0: 2, > 0: 3}, v = 0 the master, holds the output bit and trust byte of
 * _doVote2 (voters = 2, softCombiner.py:623-662) resp. _doVoteN (softCombiner.py:570-618) for that column.  Both are functions of
 * the column alone and look at trust only through these classes; the host evaluates them once per masterVoteWeight. */
int mfb_combiner_set_vote(mfb_combiner *c, int voters, const uint8_t *lut_bits, const int8_t *lut_trust, int entries);
/* _begin copies the streams in, enqueues everything -- pack, per slave correlation / top-15 / decision, vote -- and returns; no
 * host synchronisation between slaves.  _end waits and hands out the record and out_len bits / trust bytes (room for master_len
 * each).  One call in flight per combiner.  MFB_ERR_ARG: lengths <= 0 or beyond max_bits, more slaves than max_slaves;
 * MFB_ERR_UNSUPPORTED: more than MFB_COMBINE_MAX_SLAVES slaves; MFB_ERR_STATE: a call in flight, _end without _begin, or a vote
 * table that the call may need is not set.  Replaces SoftCombiner.correlate's numpy loop, softCombiner.py:697-774. */
int mfb_combiner_begin(mfb_combiner *c, const mfb_combine_params *p, const uint8_t *master_bits, const int8_t *master_trust,
                       const uint8_t *const *slave_bits, const int8_t *const *slave_trust);
int mfb_combiner_end(mfb_combiner *c, mfb_combine_result *result, uint8_t *bits, int8_t *trust);
/* Test seam of the correlation: all N = 2^ceil(log2 n) lags of slave a_bits[n] against master b_bits[m] (the first min(m, n) bits
 * of it), int32 out[N]: abs(customXCorr(bitsX, bitsM[:n])), softCombiner.py:703-706.  1 <= n, m <= 2^20. */
int mfb_debug_bit_xcorr(int device, const uint8_t *a_bits, int n, const uint8_t *b_bits, int m, int32_t *out);
/* Test seam of the peak stages (softCombiner.py:709-747): what a call runs for slave 0 after its correlation -- the record's
 * initialisation with Lc = master_len, the fifteen peaks of every 4096 lags, their merge and the decision, the final status: the
 * production kernels on the production grids -- on a correlation x[nlags] of the caller's choice instead of one of bit streams; n is
 * the slave's length (avail = max(0, min(Lc, n - idx0))).  No vote: *out is the record alone.  1 <= nlags, n, master_len <= 2^20
 * (MFB_ERR_UNSUPPORTED beyond), every x[k] >= 0 (MFB_ERR_ARG). */
int mfb_debug_combine_peaks(int device, const int32_t *x, int nlags, int n, int master_len, double variance_multiplier,
                            int min_length, mfb_combine_result *out);

/* The transmit side: LUT modulation of bit frames on the device (csrc/mod_kernels.hpp).  Replaces Modulator.modulate,
 * modulator/modulator.py:97-129, with FSKmod.modulate (modulator/modulators/FSK_LUT.py:25-42) or GMSKmod.modulate
 * (modulator/modulators/GMSK_LUT.py:51-72) inside it.  The phase is a uint64 in turns: an increment of v rad is quantised once, in
 * double, as t = v / (2 pi); t -= floor(t); q = (uint64)(t * 2^64) (q = 0 should t have rounded up to 1.0); every sum after that is
 * uint64 and wraps, which is the reference's np.mod(cumsum(...), 2 pi) done exactly and independent of the order of summation.
 * Limits (MFB_ERR_UNSUPPORTED beyond): 2 <= samples per symbol <= 1024, at most 2^17 bits per frame, 4096 frames, 2^22 bits and 2^24
 * output samples per batch.
 *   mfb_modulator_create   a stream, staging and device buffers for batches of up to max_bits bits (all frames together) and
 *                          max_samples output samples (pads included).  Shaped like mfb_combiner_create.
 *   mfb_modulator_set_lut  the table of phase increments, rad per sample, double [rows][sps] -- the reference's modulatorCLS.LUT
 *                          WITHOUT Doppler and offsets (those are per frame, below), uploaded once.  MFB_MOD_FSK: rows = 2, row = the
 *                          bit, initial phase -(2 b0 - 1) pi / 2 (FSK_LUT.py:31).  MFB_MOD_GMSK3: rows = 8, row of symbol s =
 *                          4 b[s-1] + 2 b[s] + b[s+1] with the bit before the first and after the last taken as 0 (GMSK_LUT.py:58-62),
 *                          initial phase 0, frames of at least 2 bits.
 *   mfb_modulator_set_pad  pad_len samples noise[0 .. pad_len) in front of and behind every frame (modulator.py:117-118); a frame
 *                          that is then shorter than min_len gets noise[0 .. min_len - length) in front of that (modulator.py:121-123).
 *                          noise_iq: noise_len complex64, noise_len >= max(pad_len, min_len).  pad_len = 0 and min_len = 0 (the
 *                          state after create): no padding, noise_iq may be NULL.
 *   mfb_modulator_begin    B frames: bits uint8 0/1 [bit_off[B]], frame f = bits[bit_off[f] .. bit_off[f+1]), bit_off[0] = 0;
 *                          dphi_rad[f] = the frame's Doppler + offset increment in rad per sample, dopplerCoef + offsetCoef of
 *                          modulator.py:103-108 (NULL: all 0).  Copies in, enqueues the three kernels and returns.
 *   mfb_modulator_end      waits; sample_off int64 [B+1] (may be NULL) receives where each frame starts in the output, sample_off[B]
 *                          the total; out_iq (may be NULL: the batch stays on the device) receives sample_off[B] complex64 -- a
 *                          plain DMA when it is the buffer of mfb_modulator_host_buffer.
 *   mfb_modulator_device_output   the last finished batch on the device (complex64) and its length, valid until the next _begin: a
 *                          frame of it is what mfb_upload_device takes.
 *   mfb_modulator_host_buffer     page-locked room for max_samples complex64, owned by the handle.
 * Misuse is an error code, never a fault.  MFB_ERR_ARG: NULL where not allowed, B < 1, offsets not increasing (a frame of 0 bits),
 * a GMSK frame of < 2 bits, more bits or samples than the handle was created for; MFB_ERR_STATE: no LUT set, _begin or a setter
 * while a call is in flight, _end without _begin, an accessor before the first batch has ended. */
#define MFB_MOD_FSK   0
#define MFB_MOD_GMSK3 1
typedef struct mfb_modulator mfb_modulator;
int mfb_modulator_create(mfb_modulator **out, int device, int max_bits, int max_samples);
int mfb_modulator_destroy(mfb_modulator *m);
int mfb_modulator_set_lut(mfb_modulator *m, int kind, const double *lut_rad, int rows, int sps);
int mfb_modulator_set_pad(mfb_modulator *m, const float *noise_iq, int noise_len, int pad_len, int min_len);
int mfb_modulator_begin(mfb_modulator *m, const uint8_t *bits, const int32_t *bit_off, const double *dphi_rad, int B);
int mfb_modulator_end(mfb_modulator *m, float *out_iq, int64_t *sample_off);
int mfb_modulator_device_output(mfb_modulator *m, const void **dev_c64, int64_t *nsamples);
int mfb_modulator_host_buffer(mfb_modulator *m, float **host_iq);
/* Test seam: the uint64 phase word of every output sample of the last finished batch (0 in the pads), words [capacity >=
 * sample_off[B]].  The words come from the production kernels on the production grids: the sample kernel is launched once more on
 * the batch's rows and scan, and writes them out beside the samples.  No reference counterpart (its phase is a float64 cumsum,
 * FSK_LUT.py:31, and is never handed out). */
int mfb_debug_mod_phase(mfb_modulator *m, uint64_t *words, int64_t capacity);

typedef struct mfb_channel mfb_channel;
typedef struct mfb_channel_params {
    int64_t base;             /* absolute position of the window's first sample */
    int64_t mute_before;      /* absolute positions below it are +0 (0: none) */
    uint64_t seed;
    int32_t count;
    int32_t buffer;           /* 0 or 1 */
    float sigma;              /* standard deviation per component */
    float adc_scale;
    int32_t adc_bits;
    int32_t reserved;
} mfb_channel_params;
typedef struct mfb_channel_frame {
    int64_t start;            /* absolute position of the frame's first sample */
    int64_t src;              /* its first sample in the source */
    int32_t length;
    float gain;
    uint64_t phase0;          /* carrier phase at its first sample, turns * 2^64 */
    uint64_t freq;            /* turns * 2^64 per sample at its first sample */
    uint64_t rate;            /* turns * 2^64 per sample, per sample */
} mfb_channel_frame;
/* The channel between the two ends, on the device (csrc/channel_kernels.hpp): frames placed at their arrival times in one
 * continuous stream, each on its own carrier with a linear frequency drift, white Gaussian noise underneath, optionally an ADC's
 * grid.  Restates awgn (examples/benchmark/create_signals.py:115-141) and the zero pad and mix of get_padded_packet
 * (create_signals.py:197-198); the "N copies of one packet, fresh noise each" of the reference's bench_modem.py is N descriptors
 * that name the same source span.  One call renders `count` samples, the absolute positions base .. base + count, and the stream
 * is a pure function of (seed, frames, source, parameters, absolute position): a span rendered in one call equals the same span
 * rendered in any number of calls, bit for bit.  Per absolute sample n:
 *     out[n] = adc(gain_f src[src_f + k] e^{2 pi i phi_f(k) / 2^64} + sigma (gI(n) + i gQ(n)))   k = n - start_f, frame f covers n
 *     out[n] = adc(sigma (gI(n) + i gQ(n)))                                                      no frame covers n
 *     out[n] = +0 + 0i                                                                           n < mute_before
 * phi_f(k) = phase0 + k freq + (k (k - 1) / 2) rate in uint64 turns modulo 2^64 (the modulator's convention above; the caller
 * quantises the three values once by the same rule, a negative one as the two's complement of its magnitude); a phase word of 0 is
 * exactly (1, 0).
 * Noise: Philox4x32-10, key = the halves of seed, counter = (n >> 1, 0, 0), sample n taking words 2 (n & 1) and 2 (n & 1) + 1;
 * u = ((w >> 8) + 1) 2^-24, radius sqrt(-2 ln u) <= 5.77, the second word the angle.  adc_bits 0 (none), 8 or 16 with adc_scale a
 * power of two: rint(x / scale) to even, saturated, times scale -- what MFB_SAMPLES_SC8 / _SC16 compute from the integers.
 *   mfb_channel_create     a stream, two output windows of max_samples complex64, device room for max_source source samples and
 *                          max_frames descriptors, page-locked staging.  Shaped like mfb_modulator_create.
 *   mfb_channel_set_source what the frames read: nsamples complex64.  on_device = 0: host samples, copied in (at most max_source);
 *                          1: a device pointer used in place, for example mfb_modulator_device_output's -- the caller keeps it
 *                          alive and unchanged while renders use it.
 *   mfb_channel_begin      enqueues one window into buffer params->buffer (0 or 1) and returns.  frames[nframes] sorted by start,
 *                          not overlapping, each reading source[src .. src + length); a frame may begin before base or end after
 *                          base + count (it is clipped); nframes = 0: noise alone, frames may be NULL.
 *   mfb_channel_end        waits; out_iq (may be NULL: the window stays on the device) receives count complex64.
 *   mfb_channel_device_output   the window rendered last into `buffer`: what mfb_receive_blocks_begin takes with MFB_INPUT_DEVICE.
 *                          Valid until the next _begin on that buffer.  The pointer is 16-byte aligned for an even base, 8-byte
 *                          aligned for an odd one.
 * Misuse is an error code, never a fault.  MFB_ERR_ARG: NULL where not allowed, count < 1, a negative base or start, a length < 1,
 * frames not sorted by start or overlapping, a frame reading outside the source, a sigma or gain that is not finite, an
 * adc_bits or adc_scale outside the above, more samples, source or frames than the handle was created for; MFB_ERR_STATE: _begin
 * or _set_source while a call is in flight, _end without _begin, frames given while no source is set, _device_output of a buffer
 * never rendered.  Limits (MFB_ERR_UNSUPPORTED beyond): 2^24 samples per window, 2^26 source samples, 2^20 frames, base < 2^62. */
int mfb_channel_create(mfb_channel **out, int device, int max_samples, int max_source, int max_frames);
int mfb_channel_destroy(mfb_channel *c);
int mfb_channel_set_source(mfb_channel *c, const void *samples_c64, int64_t nsamples, int on_device);
int mfb_channel_begin(mfb_channel *c, const mfb_channel_params *params, const mfb_channel_frame *frames, int nframes);
int mfb_channel_end(mfb_channel *c, float *out_iq);
int mfb_channel_device_output(mfb_channel *c, int buffer, const void **dev_c64, int64_t *nsamples);
/* Test seam of the noise: npairs pairs of 32-bit words (first word -> radius, second -> angle) through the production device
 * function, out = npairs (gI, gQ) float pairs.  Reaches the ends of the uniform without a search for seeds.  No reference
 * counterpart (the reference draws from numpy's generator, create_signals.py:115-141). */
int mfb_debug_channel_normals(int device, const uint32_t *words, int npairs, float *out);

/* HIP-event stopwatch on the handle's stream (bench.py's live kernel timing).  The reference times blocks with time.time()
 * around the whole call (DP:324-333). */
int mfb_timer_start(mfb_ctx *ctx);
int mfb_timer_stop(mfb_ctx *ctx, float *elapsed_ms);
/* Per-kernel accounting: when enabled, every launch of the search kernels is bracketed by HIP
 * events on the handle's stream; mfb_profile_read synchronises and returns launch counts and
 * summed milliseconds, then clears them: slot 0 = pass 1 (two-pass) or the segment kernel,
 * slot 1 = pass 2 (two-pass; stays 0 on the segment path).  No reference counterpart (the reference logs block rates only,
 * DP:324-333). */
int mfb_profile_enable(mfb_ctx *ctx, int on);
int mfb_profile_read(mfb_ctx *ctx, int counts[2], float total_ms[2]);
/* Block until all work enqueued on the handle's stream has finished (the reference: cuda.Context.synchronize(), DB:651). */
int mfb_sync(mfb_ctx *ctx);

#define MFB_SAMPLES_CF32 0   /* interleaved float pairs */
#define MFB_SAMPLES_SC16 1   /* interleaved int16 I, Q, native endianness */
#define MFB_SAMPLES_SC8  2   /* interleaved int8 I, Q */
/* Integer IQ samples as the radio delivers them, converted on the device.  The reference's demodulator takes complex64 only
 * (integers off a socket appear in its tree only as decoded bits: np.frombuffer(..., np.int8), examples/benchmark/bench_modem.py:134):
 * whoever feeds it converts on the host first and copies 8 bytes per sample into the page-locked buffer (DB:456-457, DP:256,287,337).
 * mfb_set_sample_format sets the element type of the handle's page-locked inputs -- the two one-block input buffers and the two
 * batch windows: the caller fills them with interleaved int16 or int8 I, Q pairs, 4 or 2 bytes per sample cross the host link, and a
 * kernel behind the copy (csrc/unpack_kernels.hpp) writes complex64 = integer * scale into the device copy that everything else
 * reads.  Blocks in device memory (MFB_INPUT_DEVICE) and mfb_upload_device stay complex64 always.
 *   scale      the value of one integer step.  0: full scale 1.0 (2^-15 for sc16, 2^-7 for sc8); else a positive, finite power of
 *              two (frexpf mantissa exactly 0.5) for which every sample stays a normal float: MFB_ERR_ARG otherwise.  An int16 /
 *              int8 converts to float32 without rounding and a multiplication by a power of two is exact, so every sample is bit for
 *              bit what raw.astype(float32) * scale gives on the host -- and so is everything computed from it.  Other gains are
 *              refused for that reason.
 * Unknown format: MFB_ERR_ARG; anything in flight: MFB_ERR_STATE; after a refusal the previous format stays in force.  A change
 * synchronises, drops the recorded graphs, restarts the peak-clip chain (as mfb_restart_peak_clip) and zero-fills the page-locked
 * inputs.  While the format is not CF32: mfb_input_buffer, mfb_input_buffer2 and mfb_window_buffer return MFB_ERR_STATE (use the
 * _raw calls below), mfb_upload_from (complex64 host data) returns MFB_ERR_UNSUPPORTED; mfb_upload, the pinned buffer, honours
 * the format. */
int mfb_set_sample_format(mfb_ctx *ctx, int format, float scale);
/* What is in force (any pointer may be NULL): 8, 4 or 2 bytes per sample.  No reference counterpart (complex64 only, DB:456-457). */
int mfb_get_sample_format(mfb_ctx *ctx, int *format, float *scale, int *bytes_per_sample);
/* The page-locked input buffer of mfb_input_buffer (which = 0) / mfb_input_buffer2 (which = 1) typed by the format in force:
 * N samples of it, *bytes = N * bytes_per_sample (the allocation keeps its complex64 size; only those bytes are used).  Replaces
 * pagelocked_empty(...) DB:456-457 / get_signalBufferHostPointer DB:1055-1060 for integer samples. */
int mfb_input_buffer_raw(mfb_ctx *ctx, int which, void **host, size_t *bytes);
/* mfb_window_buffer likewise: the window of max_blocks * block_stride + (N - block_stride) samples of the format in force -- the
 * destination of the loop's copies (DP:256,287,337). */
int mfb_window_buffer_raw(mfb_ctx *ctx, int which, int max_blocks, int block_stride, void **host, size_t *bytes);
/* Test seam of the conversion: the kernel behind the copies on nsamples host samples of `format` (SC16 / SC8; scale as for
 * mfb_set_sample_format), out_c64 = nsamples complex64.  The product paths do not use it.  No reference counterpart (its
 * callers convert with numpy on the host). */
int mfb_debug_unpack(int device, int format, float scale, const void *raw, size_t nsamples, float *out_c64);

typedef struct mfb_channelizer mfb_channelizer;
enum { MFB_CHZ_INPUT_PINNED0 = 0, MFB_CHZ_INPUT_PINNED1 = 1, MFB_CHZ_INPUT_DEVICE = 2 };
typedef struct mfb_channelizer_params {
    int64_t in_base;          /* absolute position of the call's first input sample */
    int64_t out_base;         /* absolute position, in a channel's output stream, of the call's first output */
    const void *device_input; /* MFB_CHZ_INPUT_DEVICE: in_count samples of the plan's format in device memory, aligned to one sample */
    int32_t in_count;
    int32_t out_count;
    int32_t input;            /* MFB_CHZ_INPUT_PINNED0 / _PINNED1: the page-locked buffer of mfb_channelizer_input_buffer; _DEVICE */
    int32_t buffer;           /* output set 0 or 1 */
} mfb_channelizer_params;
/* The channeliser in front of the banks, on the device (csrc/channelize_kernels.hpp): one wideband capture, complex64 or the
 * integers a radio delivers, becomes K channels, each tuned to baseband, low-pass filtered and decimated to the rate a bank is built
 * for.  No reference counterpart: the reference takes one narrowband stream per radio process (pyCuSDR.py:245-251).
 * One plan holds a decimation D, real taps h[0..T) and K tuning words freq_k, uint64 turns * 2^64 per input sample (the modulator's
 * convention above; a negative frequency is the two's complement).  With n the absolute position in the wideband stream and m in a
 * channel's output stream:
 *     phi_k(n) = n freq_k                                                   (uint64, modulo 2^64)
 *     y_k[m]   = sum_{t < T} h[t] x[m D - t] e^{-2 pi i phi_k(m D - t) / 2^64}     x[n] = 0 for n < 0
 * computed as e^{-2 pi i phi_k(m D) / 2^64} sum_t (h[t] e^{+2 pi i phi_k(t) / 2^64}) x[m D - t], which is the same thing because phi_k
 * is linear in integers.  x is complex64; for MFB_SAMPLES_SC16 / _SC8 it is float(int) * scale with scale a power of two (0: full
 * scale 1.0, as mfb_set_sample_format).  y_k[m] is a pure function of (h, D, freq_k, the T samples it reads, m): a span computed in
 * one call equals the same span computed in any number of calls, from any input window that covers it, beside any other channels,
 * bit for bit.  freq_k = 0 filters with h itself and rotates nothing; a rotation word of 0 multiplies nothing: h = [1], freq = 0
 * gives y[m] = x[m D] bit for bit.  The group delay of a symmetric h is (T - 1) / 2 input samples.
 *   mfb_channelizer_create         a stream, two output sets of max_channels x max_out complex64, a tap table.
 *   mfb_channelizer_set_plan       D, the taps, the words, the sample format; builds the tap tables on the device and waits.
 *   mfb_channelizer_input_buffer   page-locked staging `which` (0 or 1) in the plan's sample format, allocated on first use for max_in
 *                                  samples: *bytes = max_in * bytes per sample.  Needs a plan.
 *   mfb_channelizer_begin          enqueues one call and returns: inputs [in_base, in_base + in_count) -> outputs [out_base, out_base +
 *                                  out_count) of every channel, into output set `buffer`.
 *   mfb_channelizer_end            waits; out_c64 (may be NULL: the outputs stay on the device) receives [nchan][out_count] complex64.
 *   mfb_channelizer_device_output  channel `channel` of the call that wrote output set `buffer` last: 16-byte aligned complex64, what
 *                                  mfb_upload_device and MFB_INPUT_DEVICE take.  Valid until the next _begin on that set or _set_plan.
 *   mfb_channelizer_info           outputs_per_workgroup: the tile of the plan in force (64, 128 or 256); taps_capacity: max_taps.
 *   mfb_channelizer_elapsed_ms     device time of the call finished last (events around its kernel, copies of pinned input excluded).
 * Misuse is an error code, never a fault.  MFB_ERR_ARG: NULL where not allowed, counts < 1, negative bases, a buffer outside 0 / 1,
 * an unknown format or input, a scale that is not a power of two, taps that are not finite, a device pointer not aligned to a
 * sample, more channels, taps, inputs or outputs than the handle was created for, and an output range whose inputs
 * [out_base D - (T - 1), (out_base + out_count - 1) D] are not all inside [in_base, in_base + in_count), apart from positions below 0,
 * which read as zero.  MFB_ERR_STATE: _begin or _set_plan while a call is in flight, _end without _begin, _begin, _info or
 * _input_buffer without a plan, a pinned input whose buffer was never asked for, _device_output of a set never written or of a
 * channel outside the plan that wrote it.  Limits (MFB_ERR_UNSUPPORTED beyond): 1..16 channels, D in 2..64, 1..1024 taps, 2^24 input
 * and 2^22 output samples per channel and call, in_base and out_base D < 2^62. */
int mfb_channelizer_create(mfb_channelizer **out, int device, int max_channels, int max_taps, int max_in, int max_out);
int mfb_channelizer_destroy(mfb_channelizer *c);
int mfb_channelizer_set_plan(mfb_channelizer *c, int decim, const float *taps, int ntaps, const uint64_t *freq_words, int nchan,
                             int sample_format, float sample_scale);
int mfb_channelizer_input_buffer(mfb_channelizer *c, int which, void **host, size_t *bytes);
int mfb_channelizer_begin(mfb_channelizer *c, const mfb_channelizer_params *params);
int mfb_channelizer_end(mfb_channelizer *c, float *out_c64);
int mfb_channelizer_device_output(mfb_channelizer *c, int buffer, int channel, const void **dev_c64, int64_t *nsamples);
int mfb_channelizer_info(mfb_channelizer *c, int *outputs_per_workgroup, int *taps_capacity);
int mfb_channelizer_elapsed_ms(mfb_channelizer *c, float *ms);
/* Rational resampling in the channeliser (csrc/channelize_rational_kernels.hpp): a plan that resamples every channel by U / D
 * instead of decimating it by D, for capture rates that are no integer multiple of the bank's.  No reference counterpart: the
 * reference takes one narrowband stream at the bank's own rate (pyCuSDR.py:245-251).
 * The plan holds an interpolation U = interp and a decimation D = decim, real taps h[0..T) given at the virtual rate U fs, and K
 * tuning words freq_k, uint64 turns * 2^64 per INPUT sample.  With n the absolute input position and m the absolute output position:
 *     q(m) = (m D) div U        r(m) = (m D) mod U
 *     y_k[m] = sum over j >= 0 with r + jU < T of
 *              h[r + jU] x[q - j] e^{-2 pi i phi_k(q - j) / 2^64}      phi_k(n) = n freq_k mod 2^64,  x[n] = 0 for n < 0
 * the zero-stuff, filter, keep-every-D-th definition restricted to the products that are not zero, computed as
 *     e^{-2 pi i phi_k(q) / 2^64} * sum_j g_k[r + jU] x[q - j]        g_k[t] = h[t] e^{+2 pi i phi_k(t div U) / 2^64}
 * which is exact because phi_k is linear in integers.  One lane makes one output; the sum starts from (-0, -0); terms are added in
 * the order j = 0, 1, ...: for each tap the x.re terms, then the x.im terms; freq_k == 0 uses h itself with one real multiply-add
 * per component and is not rotated; a rotation word of 0 multiplies nothing.  A branch runs its own ceil((T - r) / U) taps and no
 * padded ones.  y_k[m] is a pure function of (h, U, D, freq_k, the samples it reads, m): any cut of a span, any input window that
 * covers it, any other channels in the plan and either output set give the same bits.  With U = 1 the definition is
 * mfb_channelizer_set_plan's and the bits are the same, but this call always selects the rational kernel, also at interp = 1;
 * mfb_channelizer_set_plan keeps its own.
 * Every other call of the handle works as above under such a plan, with two differences.  mfb_channelizer_begin: the outputs
 * [out_base, out_base + out_count) read the inputs [q(out_base) - (ceil(T / U) - 1), q(out_base + out_count - 1)] -- the uniform
 * bound, one sample generous for short branches -- which must all lie inside [in_base, in_base + in_count), apart from positions
 * below 0, which read as zero: MFB_ERR_ARG otherwise.  mfb_channelizer_info: outputs_per_workgroup is the number of consecutive
 * outputs one workgroup makes, U times 64, 128 or 256.
 * Limits (MFB_ERR_UNSUPPORTED beyond): 1 <= U <= 32, 2 <= D <= 64, T <= 1024, 1..16 channels, 2^24 inputs and 2^22 outputs per call,
 * in_base and out_base D < 2^62.  MFB_ERR_ARG: a common factor of U and D, U >= D (net rate reduction only), T < U (every branch
 * has at least one tap), and everything mfb_channelizer_set_plan refuses with it.  Misuse is an error code, never a fault. */
int mfb_channelizer_set_plan_rational(mfb_channelizer *c, int interp, int decim, const float *taps, int ntaps, const uint64_t *freq_words,
                                      int nchan, int sample_format, float sample_scale);
/* The uniform polyphase channeliser (csrc/channelize_uniform_kernels.hpp): the channels of a raster, bin k of M centred on k fs / M,
 * all made by one M-point transform per output frame instead of one T-tap filter per channel.  No reference counterpart: the
 * reference takes one narrowband stream per radio process (pyCuSDR.py:245-251).
 * The definition is mfb_channelizer_set_plan's with the exact words freq_k = k 2^64 / M (M a power of two), for which it collapses:
 *     y_k[m] = sum_{t < T} h[t] x[m D - t] e^{-2 pi i k (m D - t) / M}                   x[n] = 0 for n < 0
 *            = sum_{s < M} v_m[s] e^{+2 pi i k s / M}
 *     u_m[p] = sum_{j : p + j M < T} h[p + j M] x[m D - p - j M]        p = 0 .. M - 1   (M branch sums, real taps)
 *     v_m[s] = u_m[(s + m D) mod M]                                                      (a circular shift, no multiply)
 * A branch sum starts from (-0, -0) and adds its terms in the order j = 0, 1, ..., one fused multiply-add per component and tap,
 * exactly the taps with p + j M < T; the transform's order of operations is a function of M alone.  So y_k[m] is a pure function of
 * (h, D, M, the T samples it reads, m): any cut of a span, any input window that covers it, any selection of bins and either
 * output set give the same bits.  Against the float64 definition every component is within (ceil(T / M) + 3 log2 M + 2) 2^-24 S_m,
 * S_m = sum_t |h[t]| |x[m D - t]|.  Adjacent bins overlap as the taps dictate; D need not divide M, critical sampling is D = M.
 *   mfb_channelizer_create_uniform    a handle of the same type for nbins = M bins of which at most max_selected are written: a
 *                                     stream, two output sets of max_selected x max_out complex64, the taps.
 *   mfb_channelizer_set_plan_uniform  D, the taps, the selected bins (indices in [0, M), in the order of the output's rows, no
 *                                     duplicates), the sample format and scale as mfb_channelizer_set_plan; waits.
 * Every other call works on such a handle as above: _input_buffer; _begin with the required-input rule of mfb_channelizer_set_plan,
 * [out_base D - (T - 1), (out_base + out_count - 1) D]; _end, which returns [nselected][out_count]; _device_output, where `channel`
 * indexes the selection; _elapsed_ms; _destroy; _info, where outputs_per_workgroup is F, the consecutive frames a workgroup makes
 * (a multiple of 16 up to 128 wherever 64 KiB of LDS hold them, else 8 or 4), and taps_capacity is max_taps.
 * The two kinds of plan do not mix, MFB_ERR_STATE: mfb_channelizer_set_plan or _set_plan_rational on a handle of
 * mfb_channelizer_create_uniform, mfb_channelizer_set_plan_uniform on a handle of mfb_channelizer_create; and _set_plan_uniform while
 * a call is in flight.  MFB_ERR_ARG: NULL where not allowed, counts < 1, an unknown format, a scale that is not a power of two,
 * taps that are not finite, a bin outside [0, M) or named twice, more taps or selected bins than the handle was created for.
 * Limits (MFB_ERR_UNSUPPORTED beyond): M one of 8, 16, 32, 64, 128, 256; 2 <= D <= M; 1..4096 taps; 1..M selected bins; 2^24 inputs
 * and 2^22 outputs per call; max_selected max_out <= 2^26 samples per output set; in_base and out_base D < 2^62.  Misuse is an
 * error code, never a fault. */
int mfb_channelizer_create_uniform(mfb_channelizer **out, int device, int nbins, int max_selected, int max_taps, int max_in, int max_out);
int mfb_channelizer_set_plan_uniform(mfb_channelizer *c, int decim, const float *taps, int ntaps, const int32_t *bins, int nselected,
                                     int sample_format, float sample_scale);
/* Rational resampling on the raster (csrc/channelize_uniform_rational_kernels.hpp): a plan of a handle of
 * mfb_channelizer_create_uniform that resamples every bin by U / D instead of decimating it by D, for capture rates that are no
 * integer multiple of the bank's (2.4 MHz -> 153.6 kHz is 8 / 125).  No reference counterpart: the reference takes one narrowband
 * stream at the bank's own rate (pyCuSDR.py:245-251).
 * The definition is mfb_channelizer_set_plan_rational's with the exact words freq_k = k 2^64 / M, for which it collapses as the
 * integer one does.  With real taps h[0..T) at the virtual rate U fs, q(m) = (m D) div U and r(m) = (m D) mod U:
 *     y_k[m] = sum_{j : r + j U < T} h[r + j U] x[q - j] e^{-2 pi i k (q - j) / M}               x[n] = 0 for n < 0
 *            = sum_{s < M} v_m[s] e^{+2 pi i k s / M}
 *     u_m[p] = sum_{i : r + (p + i M) U < T} h[r + (p + i M) U] x[q - p - i M]       p = 0 .. M - 1
 *     v_m[s] = u_m[(s + q) mod M]
 * A branch sum starts from (-0, -0) and adds its terms in the order i = 0, 1, ..., one fused multiply-add per component and tap,
 * exactly the taps with r + (p + i M) U < T; the transform is mfb_channelizer_set_plan_uniform's.  y_k[m] is a pure function of
 * (h, U, D, M, the samples it reads, m): any cut of a span, any input window that covers it, any selection of bins and either output
 * set give the same bits.  Against the float64 definition every component is within (ceil(Tb / M) + 3 log2 M + 2) 2^-24 S_m with
 * Tb = ceil(T / U) and S_m = sum_j |h[r + j U]| |x[q - j]|; where S_m = 0 the output is zero exactly.  With U = 1 the definition and
 * the bits are mfb_channelizer_set_plan_uniform's, but this call always selects the rational kernel, also at interp = 1;
 * mfb_channelizer_set_plan_uniform keeps its own.
 * Every other call of the handle works under such a plan as under a uniform one, with these differences.  The handle's max_taps
 * bounds the taps of a branch, ceil(T / U), not T.  mfb_channelizer_begin: the outputs [out_base, out_base + out_count) read the
 * inputs [q(out_base) - (Tb - 1), q(out_base + out_count - 1)], the rule of mfb_channelizer_set_plan_rational.  mfb_channelizer_info:
 * outputs_per_workgroup is F, the consecutive frames a workgroup makes under this plan (the largest that 64 KiB of LDS hold, F M a
 * multiple of 256), taps_capacity is max_taps.  The survey stays a matter of integer plans: mfb_channelizer_set_survey under such a
 * plan, and this call while a survey is set, are MFB_ERR_UNSUPPORTED.
 * Limits (MFB_ERR_UNSUPPORTED beyond): 1 <= U <= 32; 2 <= D <= U M, the output rate may not fall below the bin spacing;
 * ceil(T / U) <= 4096; 1..M selected bins; those of mfb_channelizer_begin.  MFB_ERR_ARG: a common factor of U and D, U >= D (net
 * rate reduction only), T < U (every branch has at least one tap), ceil(T / U) above the handle's max_taps, and everything
 * mfb_channelizer_set_plan_uniform refuses with it.  MFB_ERR_STATE: a handle of mfb_channelizer_create; a call in flight.  Misuse is
 * an error code, never a fault. */
int mfb_uniform_channelizer_set_plan_rational(mfb_channelizer *c, int interp, int decim, const float *taps, int ntaps,
                                              const int32_t *bins, int nselected, int sample_format, float sample_scale);
/* The survey of the raster (csrc/channelize_survey_kernels.hpp): how much power every one of the M bins of a uniform plan held in
 * each stretch of time, what the noise floor was, and which (bin, stretch) cells stand above it -- reduced on the device from the
 * frames a call makes anyway, with or without writing any of them.  No reference counterpart: the reference takes one narrowband
 * stream per radio process (pyCuSDR.py:245-251).
 * With y_k[m] the uniform plan's output for bin k = 0 .. M - 1, the very bits mfb_channelizer_begin would write:
 *     cell      L = cell_frames = 2^l frames, 2 <= l <= 16; cell s of bin k covers the output positions [s L, (s + 1) L).
 *     p_k[m]  = fl(fl(re re) + fl(im im)), float32, not fused.
 *     P[s][k] = the balanced pairwise sum of the L values p_k[s L .. s L + L): at each level q[i] = fl(q[2 i] + q[2 i + 1]).
 *     floor[s] = the rank-th smallest (0-based) of the M values P[s][.], 0 <= rank < M: an exact selection.  M / 4 stays on noise
 *               while fewer than three quarters of the raster are occupied.
 *     mask      bit (s, k) is set iff P[s][k] > fl(threshold floor[s]), threshold a finite float32 >= 1; packed as
 *               uint32 mask[s][ceil(M / 32)], bit j of word w being bin 32 w + j, unused bits zero.
 * k runs in natural bin order.  Every aligned power-of-two run of frames is a subtree of the sum, so P[s][k] is a pure function of
 * (plan, samples read, s, k): a span of cells computed in one call equals the same cells under any cut, from any input window that
 * covers them, in either output set, whatever bins are selected and whether or not outputs are written, bit for bit.
 *   mfb_channelizer_set_survey    on a handle of mfb_channelizer_create_uniform with a plan: the cell length, the rank and the
 *                                 threshold of the calls to come; allocates the partial sums, the two tables and the mask.
 *                                 cell_frames = 0 turns the survey off and frees them.  mfb_channelizer_set_plan_uniform drops it.
 *   mfb_channelizer_survey_info   what is set (cell_frames 0: nothing) and frames_per_workgroup, the consecutive frames a workgroup
 *                                 of a survey call makes: the largest power of two that is at most the plan's F and fits its LDS
 *                                 budget.  Any pointer may be NULL.
 *   mfb_channelizer_survey_begin  mfb_channelizer_begin plus the survey of the cells out_base / L .. (out_base + out_count) / L, in
 *                                 the same launch, and one small launch that finishes the tables, all inside the events of
 *                                 mfb_channelizer_elapsed_ms.  write_outputs = 0: no bin is written and output set `buffer` counts as
 *                                 never written.
 *   mfb_channelizer_survey_end    waits; out_c64 as mfb_channelizer_end, power [ncells][M], floor [ncells] and
 *                                 mask [ncells][ceil(M / 32)] receive the tables.  Any of the four may be NULL.
 * mfb_channelizer_begin / _end work unchanged on a handle with a survey set.  MFB_ERR_ARG: everything mfb_channelizer_begin refuses
 * with it; out_base or out_count not a multiple of L; a cell length that is no power of two in 4 .. 65536 or longer than max_out;
 * a rank outside [0, M); a threshold below 1 or not finite; out_c64 where nothing was written (the call stays in flight).
 * MFB_ERR_STATE: any of these on a handle of mfb_channelizer_create; _set_survey or _survey_info without a plan; _set_survey while a
 * call is in flight; _survey_begin without a survey set; _survey_end behind mfb_channelizer_begin, mfb_channelizer_end behind
 * _survey_begin.  Limits (MFB_ERR_UNSUPPORTED beyond, with those of mfb_channelizer_begin): M out_count <= 2^26 and
 * M out_count / L <= 2^22 table entries per call.  Misuse is an error code, never a fault. */
int mfb_channelizer_set_survey(mfb_channelizer *c, int cell_frames, int rank, float threshold);
int mfb_channelizer_survey_info(mfb_channelizer *c, int *cell_frames, int *frames_per_workgroup, int *rank, float *threshold);
int mfb_channelizer_survey_begin(mfb_channelizer *c, const mfb_channelizer_params *params, int write_outputs);
int mfb_channelizer_survey_end(mfb_channelizer *c, float *out_c64, float *power, float *floor, uint32_t *mask);

typedef struct mfb_synthesizer mfb_synthesizer;
typedef struct mfb_synthesizer_params {
    int64_t out_base;         /* absolute wide position of the call's first output */
    int32_t out_count;
    int32_t buffer;           /* 0 or 1: the output set the call writes */
} mfb_synthesizer_params;
typedef struct mfb_synthesizer_placement {
    int64_t start;            /* absolute position of the first sample in the bin's narrow stream */
    int64_t src;              /* its first sample in the source */
    int32_t length;
    int32_t bin;              /* 0 .. M - 1 */
    float gain;
    int32_t reserved;
} mfb_synthesizer_placement;
/* The uniform polyphase synthesiser (csrc/synthesize_uniform_kernels.hpp), the dual of mfb_channelizer_create_uniform: narrowband
 * streams are put onto the M bins of a raster of one wideband stream, each interpolated by I, filtered with the plan's real taps and
 * mixed to b fs / M, all with one M-point transform per input frame.  No reference counterpart: the reference makes one narrowband
 * stream per radio process (pyCuSDR.py:245-251).
 * x_b[m] = fl(gain source[src + m - start]) (float32, one rounding per component; a gain of 1 multiplies nothing) where a placement
 * of bin b covers m, 0 elsewhere.  With n the absolute wide position and (q, r) = divmod(n, I):
 *     w[n] = sum_b e^{+2 pi i b n / M} sum_{j >= 0, r + j I < T} h[r + j I] x_b[q - j]
 *          = sum_{j >= 0, r + j I < T} h[r + j I] X_{q - j}[n mod M]          X_m[s] = sum_b x_b[m] e^{+2 pi i b s / M}
 * zero-stuff by I, filter, mix to the exact word b 2^64 / M, without the zero products.  Each output starts from (-0, -0) and adds
 * j = 0, 1, ... in order, one fused multiply-add per component and tap; w[n] is a pure function of (h, I, M, the placements, n): a
 * span equals itself under any cut into calls, in either output set, bit for bit.
 *   mfb_synthesizer_create         a stream, two output sets of max_out complex64, a tap table of max_taps, device room for
 *                                  max_source source samples and max_frames placements, page-locked staging for the placements.
 *   mfb_synthesizer_set_plan       I and the taps (wide rate); waits.  2 <= I <= M, I need not divide M.
 *   mfb_synthesizer_set_source     what the placements read, as mfb_channel_set_source: host samples are copied in (at most
 *                                  max_source), device memory is used in place and stays the caller's.
 *   mfb_synthesizer_begin          enqueues the outputs [out_base, out_base + out_count) into output set params->buffer and returns.
 *                                  placements[n] in any order; those of one bin must not overlap (abutting is allowed); each reads
 *                                  source[src .. src + length); n = 0: zeros, placements may be NULL.
 *   mfb_synthesizer_end            waits; out_c64 (may be NULL: the outputs stay on the device) receives out_count complex64.
 *   mfb_synthesizer_device_output  the call that wrote output set `buffer` last: 16-byte aligned complex64, what
 *                                  mfb_channelizer_begin takes with MFB_CHZ_INPUT_DEVICE and mfb_channel_set_source with on_device.
 *                                  Valid until the next _begin on that set.
 *   mfb_synthesizer_info           frames_per_workgroup: the F input frames whose F I outputs a workgroup makes; rows: the
 *                                  F + ceil(T / I) - 1 frames it transforms for them.  Either pointer may be NULL.
 *   mfb_synthesizer_elapsed_ms     device time of the call finished last (events around its kernel).
 * Misuse is an error code, never a fault, and launches nothing.  MFB_ERR_ARG: NULL where not allowed, counts < 1, a negative
 * out_base, start or src, a length < 1, a bin outside [0, M), a gain or tap that is not finite, a placement reading outside the
 * source, overlapping placements on one bin, a buffer outside 0 / 1, more taps, outputs, source samples or placements than the
 * handle was created for.  MFB_ERR_STATE: _begin, _set_plan or _set_source while a call is in flight, _begin before a plan or a
 * source, _info without a plan, _end without _begin, _device_output of a set never written or in flight, _elapsed_ms before a call
 * has finished.  Limits (MFB_ERR_UNSUPPORTED beyond): M one of 8, 16, 32, 64, 128, 256; 2 <= I <= M; 1..4096 taps; 2^24 outputs per
 * call, 2^26 source samples, 4096 placements; out_base and start < 2^62; a plan whose smallest tile, ceil(T / I) frames of M + 1
 * complex64 beside the table and the taps, does not fit 64 KiB of LDS -- every plan with ceil(T / I) <= 17 fits. */
int mfb_synthesizer_create(mfb_synthesizer **out, int device, int nbins, int max_taps, int max_out, int max_source, int max_frames);
int mfb_synthesizer_destroy(mfb_synthesizer *s);
int mfb_synthesizer_set_plan(mfb_synthesizer *s, int interp, const float *taps, int ntaps);
int mfb_synthesizer_set_source(mfb_synthesizer *s, const void *samples_c64, int64_t nsamples, int on_device);
int mfb_synthesizer_begin(mfb_synthesizer *s, const mfb_synthesizer_params *params, const mfb_synthesizer_placement *placements, int n);
int mfb_synthesizer_end(mfb_synthesizer *s, float *out_c64);
int mfb_synthesizer_device_output(mfb_synthesizer *s, int buffer, const void **dev_c64, int64_t *nsamples);
int mfb_synthesizer_info(mfb_synthesizer *s, int *frames_per_workgroup, int *rows);
int mfb_synthesizer_elapsed_ms(mfb_synthesizer *s, float *ms);

/* Test seams of the demodulation tail: the three kernels between the matched filters and the bit stream, launched as the product
 * launches them, on INJECTED inputs (tests/test_gpu_demod_tail.py).  Handle-less: device buffers of their own, a synchronous copy
 * back; the product paths do not use them.  MFB_ERR_UNSUPPORTED: more than 2^26 complex64 input elements.
 *   mfb_debug_envelope   sumXCorrBuffMasks (CU:191-205) on xc complex64 [nb][M][N]: env float32 [nb][N], env[b][n] = sum over
 *                        filters off <= m < M - off of |xc[b][m][n]|^2, on the grid mfb_demodulate uses (1024 x nb workgroups of 256).
 *                        Any N >= 1; off as mfb_create's code_search_mask_offset (0 <= 2 * off < M).
 *   mfb_debug_code_rate  findCodeRateAndPhase (CU:236-320) over [offset, offset + len) of each of the nb windows P complex64 [nb][n],
 *                        twice: the kernel of mfb_demodulate once per window -> triples float32 [nb][3] = {k*, arg P[k*], |P[k*]|^2};
 *                        the one-launch form of mfb_receive_block(s) over all nb windows (block length n, records 256 bytes apart)
 *                        -> block_triples [nb][3], and what it derives per window (DB:733-752, 994-999): rate double [nb][2] =
 *                        {spSym, codeOffset}, launch_args float32 [nb][2] = the two arguments of findCentres, counts int32 [nb][2] =
 *                        {symbol count, rate_fallback}.  0 <= offset, 0 <= len, offset + len <= n as mfb_demodulate demands.
 *   mfb_debug_centres    findCentres (CU:78-146) on sig complex64 [M][lenSig] with nthreads threads in workgroups of 256.  The three
 *                        outputs hold ceil(nthreads / 256) * 256 entries each, every byte 0x5a before the launch: what the kernel
 *                        does not write (entries from `capacity` on) comes back as 0x5a5a5a5a.  spSym >= 2 as mfb_find_centres
 *                        demands, offset >= 0, op 0..2, nthreads <= 2^20, lenSig <= 2^22. */
int mfb_debug_envelope(int device, const float *xc_c64, int nb, int M, int N, int off, float *env);
int mfb_debug_code_rate(int device, const float *P_c64, int nb, int n, int offset, int len, int spsym_min, int capacity, float *triples,
                        float *block_triples, double *rate, float *launch_args, int32_t *counts);
int mfb_debug_centres(int device, const float *sig_c64, int M, int lenSig, int W, int op, float spSym, float offset, int capacity,
                      int nthreads, int32_t *sym, int32_t *centres, float *magnitude);

/* A host copy worker for the receive loop: the reference's loop copies every chunk of samples twice on its one thread, into the
 * ring buffer (sigFIFO.py:62-84) and from there into the page-locked input buffer (`raw[ov:] = sigIn.getBlock()`, DP:287,337).
 * Here a chunk is copied once, into the sample window of its batch (mfb_window_buffer) -- and with this worker that copy runs on a
 * thread of its own while the caller's thread does the host stages of the previous batch.  No GPU involved (plain memory; usable
 * before any handle exists).  mfb_hostcopy_submit returns at once; copies run in submission order; source and destination must
 * stay valid and untouched until mfb_hostcopy_drain has returned.  One submitting thread per worker.  (Round 6 tried two and three
 * worker threads: no gain -- 1363 ... 1432 Msamples/s with one, 1360 ... 1419 with two, 1248 ... 1346 with three at 2^15 x 64 x 32 blocks
 * per call --, the loop is bound by its own thread, not by the copies.) */
typedef struct mfb_hostcopy mfb_hostcopy;
int mfb_hostcopy_create(mfb_hostcopy **out);
int mfb_hostcopy_submit(mfb_hostcopy *q, void *dst, const void *src, size_t bytes);
int mfb_hostcopy_drain(mfb_hostcopy *q);           /* returns when every submitted copy has been made (before the batch is begun; DP:287) */
void mfb_hostcopy_destroy(mfb_hostcopy *q);        /* finishes what was submitted, then stops the thread (no reference counterpart) */

#ifdef __cplusplus
}
#endif
#endif /* MFBANK_H */
