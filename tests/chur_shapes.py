"""What the tests of the rational plans on the raster share (test_channelizer_uniform_rational_host.py,
test_gpu_channelizer_uniform_rational.py): the shapes, the error ceiling, and the frames-per-workgroup rule of
csrc/channelize_plan.hpp restated independently of the package -- the host test holds the header to it, the device test the handle."""
import numpy as np

LDS_BUDGET = 64 * 1024
# (M, U, D, T): T < U M with branches of 3 and 2 taps; a plain one; D one below U M; the 2.4 MHz -> 153.6 kHz case with
# design_taps(125, interp=8); the longest taps and the largest D, F at its smallest; long branches at a small U
SHAPES = [(8, 2, 3, 5), (8, 3, 16, 100), (16, 2, 31, 257), (64, 8, 125, 2001), (256, 32, 8191, 32 * 4096 - 5), (128, 3, 64, 3 * 4096)]


def ceiling(M, U, T):
    """c of |device - model| <= c 2^-24 S_m per component: a chain of at most ceil(Tb / M) fused multiply-adds, 3 per bit of M for
    the transform, 2 for the second order (csrc/channelize_uniform_rational_kernels.hpp)."""
    Tb = -(-T // U)
    return -(-Tb // M) + 3 * int(np.log2(M)) + 2


def brute_span(U, D, T, F):
    """The positions that F consecutive frames read, at the worst phase of the first: over one period of (m0 D) mod U."""
    Tb = -(-T // U)
    return max(((m0 + F - 1) * D) // U - (m0 * D) // U for m0 in range(U)) + Tb


def lds_bytes(M, U, D, T, F):
    return (brute_span(U, D, T, F) + F * (M + 1) + M) * 8


def ladder(M):
    """The F that the rule may give, ascending: multiples of max(16, 256 / M) up to min(128, 4096 / M), and below the first of
    them its halves down to F M = 256."""
    step = max(16, 256 // M)
    top = min(128, 4096 // M)
    return sorted(set(range(step, top + 1, step)) | {step >> s for s in range(8) if (step >> s) * M >= 256})


def plan_frames(M, U, D, T):
    """The largest F of the ladder whose span, image and table fit the budget."""
    return max(F for F in ladder(M) if lds_bytes(M, U, D, T, F) <= LDS_BUDGET)


def taps_of(rs, U, D, T):
    """design_taps(D, interp=U) where T is its length, else random taps of about unit branch gain."""
    from pycusdr_amd.channelizer import design_taps
    if T == D * 16 + 1:
        return design_taps(D, interp=U)
    return (rs.uniform(-1, 1, T) * np.sqrt(U / T)).astype(np.float32)
