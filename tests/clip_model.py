"""numpy model of the device peak clip (pycusdr_amd/csrc/clip_kernels.hpp): the reference's __thresholdInput
(demodulator/demodulator_base.py:670-707) spelled out the way numpy 2.x computes it on an x86-64 host with FMA, so that a
device result can be compared bit for bit with ``Demodulator._thresholdInput``.

  |x|    L = max(|re|, |im|), r = min / L, |x| = L * sqrt(fma(r, r, 1)) (0 for L == 0) -- numpy's SIMD complex absolute value
  mean   8192-element chunks folded in order; each chunk a balanced pairwise tree of 128-element leaves; each leaf eight strided
         accumulators combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).  mean = float32(float64(sum) / N)
  clip   t = float32(scale) * mean; x <- t * (x / |x|) in numpy's complex arithmetic; twice, round 2 on the recomputed |x|
Blocks are powers of two of at least 128 samples.
"""
import numpy as np

f32 = np.float32


def npabs(x):
    re, im = np.abs(x.real).astype(f32), np.abs(x.imag).astype(f32)
    L, S = np.maximum(re, im), np.minimum(re, im)
    with np.errstate(all='ignore'):
        r = (S / L).astype(f32)
        q = (r.astype(np.float64) ** 2 + 1).astype(f32)          # fma(r, r, 1) rounded once
        out = (L * np.sqrt(q)).astype(f32)
    out[L == 0] = 0
    inf = np.isinf(re) | np.isinf(im)
    out[inf] = np.inf
    return out


def npsum(v):
    """np.sum / np.add.reduce of a float32 vector of 2^k >= 128 elements, in numpy's order."""
    n = len(v)
    leaves = v.reshape(-1, 16, 8)
    r = leaves[:, 0, :].copy()
    for i in range(1, 16):
        r = (r + leaves[:, i, :]).astype(f32)
    s = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    s = s.astype(f32)
    per_chunk = min(64, n // 128)
    t = s.reshape(-1, per_chunk)
    while t.shape[1] > 1:
        t = (t[:, 0::2] + t[:, 1::2]).astype(f32)
    total = f32(0)
    for c in t[:, 0]:
        total = f32(total + c)
    return total


def threshold(mag, scale):
    return f32(f32(scale) * f32(np.float64(npsum(mag)) / len(mag)))


def scale_to(x, mag, t):
    """t * (x / mag) as numpy evaluates it: complex divide by (mag + 0j), then multiply by (t + 0j)."""
    z = f32(0)
    with np.errstate(all='ignore'):
        inv = (f32(1) / mag).astype(f32)
        qr = ((x.real + x.imag * z).astype(f32) * inv).astype(f32)
        qi = ((x.imag - x.real * z).astype(f32) * inv).astype(f32)
        yr = ((t * qr).astype(f32) - (z * qi).astype(f32)).astype(f32)
        yi = ((t * qi).astype(f32) + (z * qr).astype(f32)).astype(f32)
    return (yr + 1j * yi).astype(np.complex64)


def clip(x, scale):
    """Clip complex64 ``x`` in place; returns clippedPeakIPure (int64)."""
    mag = npabs(x)
    t = threshold(mag, scale)
    hot = np.flatnonzero(mag > t)
    x[hot] = scale_to(x[hot], mag[hot], t)
    mag[hot] = npabs(x[hot])
    t = threshold(mag, scale)
    hot = np.flatnonzero(mag > t)
    x[hot] = scale_to(x[hot], mag[hot], t)
    return hot.astype(np.int64)


def bursty(rng, n, bursts=20, at=()):
    """Gaussian noise with interference bursts (random places, plus the given (start, length) pairs)."""
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    places = [(int(p), int(rng.integers(1, 50))) for p in rng.integers(0, n, bursts)] + list(at)
    for p, ln in places:
        x[p:p + ln] *= f32(rng.uniform(3, 3000))
    return x


def fma3():
    try:
        from numpy._core._multiarray_umath import __cpu_features__
    except ImportError:                                   # numpy 1.x
        from numpy.core._multiarray_umath import __cpu_features__
    return bool(__cpu_features__.get('FMA3')) and bool(__cpu_features__.get('AVX512F'))
