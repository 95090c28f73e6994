"""Shared by tests/test_synthesizer_host.py and tests/test_gpu_synthesizer.py: the bins, the placements and the round-trip scene."""
import numpy as np

from pycusdr_amd.channelizer import design_taps

FS = 1.024e6
EPS = 2.0 ** -24


def ceiling(M, I, T):
    """the derived constant of csrc/synthesize_uniform_kernels.hpp: ceil(T / I) + 3 log2 M + 3"""
    return -(-T // I) + 3 * int(np.log2(M)) + 3


def analysis_ceiling(M, T):
    """the one of csrc/channelize_uniform_kernels.hpp: ceil(T / M) + 3 log2 M + 2"""
    return -(-T // M) + 3 * int(np.log2(M)) + 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def spread(M):
    """All bins, or 16 spread ones where M > 16: both ends, the middle, a neighbour of 0, and twelve more, in no order (the
    selection of tests/test_gpu_channelizer_uniform.py)."""
    if M <= 16:
        return list(range(M))
    b = [0, M - 1, M // 2, 1]
    b += [int(k) for k in np.random.RandomState(M).permutation(M) if k not in b][:12]
    return b


def noise(rs, n):
    return (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)


def two_per_bin(synth, bins, first, count):
    """Two disjoint placements on every bin over the frames first .. first + count that a call reads: the first begins 5 frames
    before them (at 0 where they begin at 0) with gain 1, the second runs 3 frames past them with gain 0.37 (the gains swap on
    odd bins); between the two lies a gap of 1 .. 3 frames, at another place on every bin, except on the first bin, whose pair
    abuts.  (placements, source length): every placement reads a span of its own."""
    out, at = [], 0
    for i, b in enumerate(bins):
        cut = first + count // 2 + (i % 5) - 2
        gap = 0 if i == 0 else 1 + i % 3
        a0, b0, b1 = first - min(first, 5), cut + gap, first + count + 3
        assert a0 < cut <= b0 < b1
        g = (1.0, 0.37) if i % 2 == 0 else (0.37, 1.0)
        out.append(synth.placement(b, a0, at, cut - a0, g[0]))
        at += cut - a0
        out.append(synth.placement(b, b0, at, b1 - b0, g[1]))
        at += b1 - b0
    return out, at


# ---- the round trip: M = 8, I = D = 4, bins 2, 6 and 4 (adjacent bins leak at 0.26 through this prototype)
RT_M, RT_I, RT_BINS, RT_FRAMES, RT_DELAY = 8, 4, (2, 6, 4), 600, 16


def round_trip_scene(seed=11):
    """(analysis taps, synthesis taps, streams complex64 [3, 600]): design_taps(4) and 4 times it; noise band-limited to 0.125
    cycles per narrow sample under a Hann^2 envelope, largest sample about 1.  The two prototypes delay by 32 wide samples each:
    16 narrow frames."""
    rs = np.random.RandomState(seed)
    h = design_taps(RT_I)
    f = np.fft.fftfreq(RT_FRAMES)
    x = np.empty((len(RT_BINS), RT_FRAMES), dtype=np.complex64)
    for k in range(len(RT_BINS)):
        spec = (rs.standard_normal(RT_FRAMES) + 1j * rs.standard_normal(RT_FRAMES)) * (np.abs(f) <= 0.125)
        s = np.fft.ifft(spec) * np.hanning(RT_FRAMES) ** 2
        x[k] = (s / np.abs(s).max()).astype(np.complex64)
    return h, (RT_I * h.astype(np.float64)).astype(np.float32), x
