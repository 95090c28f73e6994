"""The modulator's phase arithmetic on the host: a 64-bit unsigned integer in turns.

One sample's phase increment ``v`` (rad) is quantised once, in IEEE double:

    t = v / (2 pi);  t -= floor(t);  q = uint64(t * 2**64)      (q = 0 should t have rounded up to 1.0)

The product is exact (a power of two) and the conversion truncates.  Every sum after that is uint64 and wraps modulo
2**64: the reference's ``np.mod(np.cumsum(...), 2 * np.pi)`` (modulator/modulators/FSK_LUT.py:31-32, GMSK_LUT.py:67-68) done
exactly, and independent of the order of summation -- so the device kernels (csrc/mod_kernels.hpp) give the same words
whatever their grid.  This module is the ``'host'`` back end of ``Modulator`` and computes those same words with numpy.
"""
import numpy as np

FSK, GMSK3 = 0, 1                 # MFB_MOD_FSK, MFB_MOD_GMSK3 of include/mfbank.h
TWO_PI = 2 * np.pi
_U = np.uint64


def quantise(v):
    """rad -> uint64 turns, elementwise (scalars give 0-d arrays)."""
    t = np.asarray(v, dtype=np.float64) / TWO_PI
    t = t - np.floor(t)
    t = np.where(t >= 1.0, 0.0, t)
    return (t * 18446744073709551616.0).astype(np.uint64)


def rows_of(kind, bits):
    """LUT row per symbol: FSK the bit; GMSK 4 b[s-1] + 2 b[s] + b[s+1] with the bit before the first and after the last
    taken as 0 (GMSK_LUT.py:58-62)."""
    b = (np.asarray(bits) != 0).astype(np.int64)
    if kind == FSK:
        return b
    if len(b) < 2:
        raise ValueError('GMSK needs at least 2 bits')
    return 4 * np.r_[0, b[:-1]] + 2 * b + np.r_[b[1:], 0]


def initial_phase(kind, bits):
    """FSK: -(2 b0 - 1) pi / 2 (FSK_LUT.py:31); GMSK: 0."""
    if kind == FSK:
        return quantise(-(2 * int(bits[0] != 0) - 1) * np.pi / 2)
    return np.zeros((), np.uint64)


def tables(lut_rad):
    """(P, T): the in-symbol prefix sums P[r][j] = sum_{i <= j} q[r][i] and the row totals T[r] of the quantised table."""
    q = quantise(np.atleast_2d(lut_rad))
    P = np.cumsum(q, axis=1, dtype=np.uint64)
    return P, P[:, -1].copy()


def phase_words(kind, lut_rad, bits, dphi_rad=0.0):
    """The phase word of every sample of one frame, by the symbol-prefix formula the device uses:
    init + sum_{u < s} (T[row_u] + spSym d) + P[row_s][j] + (j + 1) d."""
    lut_rad = np.atleast_2d(lut_rad)
    sps = lut_rad.shape[1]
    P, T = tables(lut_rad)
    r = rows_of(kind, bits)
    d = quantise(dphi_rad)
    with np.errstate(over='ignore'):
        per = T[r] + _U(sps) * d
        base = initial_phase(kind, bits) + np.r_[_U(0), np.cumsum(per, dtype=np.uint64)[:-1]]
        return (base[:, None] + P[r] + np.arange(1, sps + 1, dtype=np.uint64)[None, :] * d).reshape(-1)


def phase_words_by_sample(kind, lut_rad, bits, dphi_rad=0.0):
    """The same words as one running sum over the samples (the reference's order)."""
    lut_rad = np.atleast_2d(lut_rad)
    q = quantise(lut_rad)
    with np.errstate(over='ignore'):
        inc = (q[rows_of(kind, bits)] + quantise(dphi_rad)).reshape(-1)
        return initial_phase(kind, bits) + np.cumsum(inc, dtype=np.uint64)


def words_to_iq(words):
    """exp(2 pi i w / 2**64) in float64 (complex128).  The word is split so that no bit of it is lost before the angle is
    formed: the top 32 bits and the rest are exact doubles."""
    w = np.asarray(words, dtype=np.uint64)
    hi = (w >> _U(32)).astype(np.float64) / 4294967296.0
    lo = (w & _U(0xFFFFFFFF)).astype(np.float64) / 18446744073709551616.0
    return np.exp(1j * TWO_PI * (hi + lo))


def pad_layout(nsig, pad_len, min_len):
    """(pre, total) of one frame: pad_len noise samples in front and behind (modulator.py:117-118), and in front of that
    noise[:min_len - length] if it is still shorter than min_len (modulator.py:121-123)."""
    total = nsig + 2 * pad_len
    pre = max(0, min_len - total)
    return pre, total + pre


def assemble(sig, noise, pad_len, min_len):
    """One frame with its pads, as the device lays it out."""
    pre, _ = pad_layout(len(sig), pad_len, min_len)
    return np.concatenate((noise[:pre], noise[:pad_len], sig, noise[:pad_len]))
