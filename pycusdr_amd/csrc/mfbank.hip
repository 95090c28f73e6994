// mfbank.hip -- hand-written gfx950 kernels + C ABI for the Doppler matched-filter bank: the library's one translation unit.
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
// This file is the translation unit: the kernel headers, then the host side in parts, each included below exactly once and in the
// order of its dependencies (no part names anything of a later one; no forward declaration holds the order together): the bank --
// bank_ctx.hpp, bank_lifecycle_api.hpp, bank_input_api.hpp, bank_search_api.hpp, bank_clip_api.hpp, bank_stream_api.hpp,
// bank_flight_api.hpp, bank_debug_api.hpp -- then the six side handles (what they share: stage_handle.hpp; with the bank: mfb_common.hpp).
// Here itself: mfb_strerror, mfb_abi_version, the N4 mfb_xcorr, the mfb_hostcopy_* shims.  Kernels live in *_kernels.hpp only.
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

// ---- the bank (mfb_ctx and everything that serves it), in dependency order
#include "bank_ctx.hpp"
#include "bank_lifecycle_api.hpp"
#include "bank_input_api.hpp"
#include "bank_search_api.hpp"
#include "bank_clip_api.hpp"
#include "bank_stream_api.hpp"
#include "bank_flight_api.hpp"
#include "bank_debug_api.hpp"

// ---- the side handles (stage_handle.hpp: what they share).  Each part is included here, once; none uses anything of the bank's.
#include "sync_api.hpp"
#include "combine_api.hpp"
#include "mod_api.hpp"
#include "channel_api.hpp"
#include "channelize_api.hpp"
#include "synthesize_uniform_api.hpp"

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

// ---- N4: bit-stream alignment cross-correlation (reference lib/customXCorr.py:5-18) -----------------
// out = ifft( fft(a, N) * conj(fft(b, N)) ) with N the handle's block length: a and b are real
// sequences, truncated or zero-padded to N exactly as np.fft.fft(a, N) does.  Built from the handle's
// forward / inverse transform passes; the handle's spectrum, filter row 0 and matched-filter buffers
// serve as scratch, so this is meant for a handle of its own (M = 1), which is how the Python helper
// uses it.
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
