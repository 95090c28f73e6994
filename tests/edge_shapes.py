"""Shapes at which the modulator's and the channeliser's kernels (csrc/mod_kernels.hpp, csrc/channelize_kernels.hpp) take the
paths the whole-chain tests never reach, shared by tests/test_edge_shapes_host.py (which proves, without a GPU, that every shape
reaches what it is listed for) and by the GPU tests that run them.

Two plain numpy emulations, written from the kernels' text and sharing no code with the package:

* ``estimate(p, D)``: the quotient both kernels take through fp32, ``q = (int)((float)p * (1.0f / (float)D))`` truncated toward
  zero, and its remainder ``p - q * D`` -- before the one-step correction, so a remainder outside [0, D) is a position at which a
  correction branch runs;
* ``chz_row_len`` / ``chz_threads``: the channeliser's choice of workgroup width (the widest of 256, 128, 64 whose LDS image of
  D rows of odd length fits 48 KiB).
"""
import itertools

import numpy as np

# ---- limits of the handles (include/mfbank.h) ----
MOD_MAX_FRAME_BITS, MOD_MAX_SAMPLES, MOD_MAX_SPS = 1 << 17, 1 << 24, 1024
MOD_TILE, MOD_WORKGROUP = 1024, 256
CHZ_MAX_DECIM, CHZ_MAX_TAPS, CHZ_LDS_BUDGET, CHZ_UNROLL = 64, 1024, 48 * 1024, 8


def estimate(p, D):
    """(q, r) of the kernels' fp32 quotient estimate of p / D, uncorrected: r < 0 or r >= D where a correction runs."""
    p = np.asarray(p, dtype=np.int64)
    assert p.size == 0 or (p.min() >= 0 and p.max() < 1 << 24)          # (float)p is exact
    rD = np.float32(1) / np.float32(D)
    q = (p.astype(np.float32) * rD).astype(np.int64)                    # one fp32 rounding, then truncation (q >= 0)
    return q, p - q * D


def chz_row_len(threads, D, T):
    span = (threads - 1) * D + T
    return ((span + D - 1) // D) | 1


def chz_threads(D, T):
    for w in (256, 128):
        if D * chz_row_len(w, D, T) * 8 <= CHZ_LDS_BUDGET:
            return w
    return 64


def chz_span(D, T):
    """positions a workgroup stages: p = 0 .. span - 1"""
    return (chz_threads(D, T) - 1) * D + T


# ---- k_mod_samples: the corrected symbol index ----
MOD_UP_SPS = (41, 47, 55, 61, 97)          # samples per symbol at which `j >= sps` runs ...
MOD_UP_BITS = (300, 2000)                  # ... in frames of either of these lengths
MOD_DOWN = (255, 33300)                    # (sps, bits) of the one frame long enough for `j < 0`: 8 491 500 samples

# ---- k_mod_scan: frame lengths (symbols) around the 4-symbols-per-thread, 1024-symbol tile ----
SCAN_LENGTHS = (2, 3, 4, 5, 255, 256, 257, 1021, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1, 1 << 17)
SCAN_SPS = 2
SCAN_DPHI = (0.0, 1.0e-3, -1.0e-6, np.pi)  # cycled over the frames; the negative one's word lies just under 2^64
SCAN_ROTATIONS = (0, 2)                    # frame i takes SCAN_DPHI[(i + rotation) % 4]

# ---- k_mod_samples: many frames in one workgroup ----
MANY_SPS = (2, 3)
MANY_FRAMES = 600


def many_frame_lengths(sps, min_bits, seed):
    """About MANY_FRAMES frame lengths of min_bits .. 5 bits whose boundaries (pad 0) fall on chosen threads of a 256-sample
    workgroup of k_mod_samples: first thread, second thread and last thread, in turn.  With sps = 2 every boundary is even, so
    there the threads are 254, 0 and 2.  Returns (lengths, residues aimed at)."""
    rs = np.random.RandomState(seed)
    residues = (255, 0, 1) if sps % 2 else (254, 0, 2)
    lengths, c = [], 0
    for want in itertools.cycle(residues):
        if len(lengths) >= MANY_FRAMES:
            break
        target = c + min_bits
        while (target * sps) % MOD_WORKGROUP != want:
            target += 1
        while c < target:
            rem = target - c
            n = int(rs.randint(min_bits, 6))
            if rem <= 5:
                n = rem
            elif rem - n < min_bits:
                n = rem - min_bits
            assert min_bits <= n <= 5
            lengths.append(n)
            c += n
    return lengths, residues


# ---- (pad, min_len) that are no multiple of anything ----
PADS = ((3, 0), (255, 0), (257, 1000), (0, 777))
PAD_SPS = 7
PAD_BITS = (10, 200, 3, 111, 2, 150)       # 10, 3 and 2 bits leave a pre-pad under either min_len, 200, 111 and 150 none

# ---- k_chz: (D, T, tile, corr): corr = the staging's `r >= D` branch runs ----
CHZ_SHAPES = (
    (23, 7, 256, False),       # last D of the wide tile, T below the unroll
    (24, 16, 128, False),      # first D of the 128-lane tile, T = two unrolls
    (41, 9, 128, True),        # T = unroll + 1
    (47, 67, 128, True),
    (40, 1024, 128, False),    # largest image of the 128-lane tile
    (41, 1024, 64, True),      # first D of the narrow tile at T = 1024
    (55, 8, 64, True),         # T = one unroll exactly
    (61, 1024, 64, True),      # largest span
)
CHZ_BOUND_FORMATS = {(47, 67): ('cf32', 'sc16'), (55, 8): ('cf32', 'sc8')}        # every other shape: cf32
CHZ_COUNT_SHAPES = ((5, 23), (47, 67))
CHZ_COUNTS = ((0, 16), (2, 2), (4, 3), (6, 7), (9, 6), (16, 0))                     # (ncplx, nreal)
CHZ_CUT_SHAPES = ((41, 9, 'cf32'), (61, 67, 'sc16'))
CHZ_ROOMY = dict(max_channels=16, max_taps=1024, max_in=1 << 16, max_out=4096, A=(47, 67, 5), B=(2, 1, 1))


def scatter_real(ncplx, nreal, seed):
    """Which of the ncplx + nreal channels are the zero-frequency ones: spread among the others, never a prefix or a suffix
    where both kinds exist, so that ChzPlan::order is a real permutation."""
    K = ncplx + nreal
    if nreal == 0 or ncplx == 0:
        return np.zeros(K, bool) if nreal == 0 else np.ones(K, bool)
    rs = np.random.RandomState(seed)
    while True:
        real = np.zeros(K, bool)
        real[rs.permutation(K)[:nreal]] = True
        order = list(np.flatnonzero(~real)) + list(np.flatnonzero(real))
        if real[0] and not real[K - 1] and order != list(range(K)):
            return real
