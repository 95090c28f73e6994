"""The yardstick of the device modulator: the integer phase model in plain numpy, written out sample by sample.

It shares no code with pycusdr_amd/modulator/: three double operations quantise an increment, a uint64 ``cumsum`` adds
them up, and float64 evaluates the result.  The device (csrc/mod_kernels.hpp) and the package's host back end must give
these words bit for bit.
"""
import numpy as np

FSK, GMSK3 = 0, 1
BOUND = 4 * 2.0 ** -24        # per component, device sample against the float64 value of its phase word (the issue's table)


def quantise(v):
    t = np.asarray(v, dtype=np.float64) / (2 * np.pi)
    t = t - np.floor(t)
    t = np.where(t >= 1.0, 0.0, t)          # a tiny negative v rounds up to 1.0: that is the turn 0
    return (t * 2.0 ** 64).astype(np.uint64)


def rows(kind, bits):
    b = (np.asarray(bits) != 0).astype(np.int64)
    if kind == FSK:
        return b
    assert len(b) >= 2
    prev = np.concatenate(([0], b[:-1]))
    nxt = np.concatenate((b[1:], [0]))
    return 4 * prev + 2 * b + nxt


def init_word(kind, bits):
    if kind == GMSK3:
        return np.uint64(0)
    return quantise(-(2 * int(np.asarray(bits)[0] != 0) - 1) * np.pi / 2)[()]


def words(kind, lut_rad, bits, dphi_rad=0.0):
    """uint64 phase word per sample: init + running sum of (q(LUT[row][j]) + q(dphi))."""
    q = quantise(np.asarray(lut_rad, dtype=np.float64))
    d = quantise(dphi_rad)
    with np.errstate(over='ignore'):
        inc = (q[rows(kind, bits)] + d).reshape(-1)
        return np.cumsum(inc, dtype=np.uint64) + init_word(kind, bits)


def iq(w):
    """exp(2 pi i w / 2^64), float64; the word split in two exact doubles first."""
    w = np.asarray(w, dtype=np.uint64)
    turns = (w >> np.uint64(32)).astype(np.float64) * 2.0 ** -32 + (w & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -64
    return np.exp(2j * np.pi * turns)


def layout(nsig, pad_len, min_len):
    """(pre, total): modulator.py:117-123 of the reference."""
    total = nsig + 2 * pad_len
    pre = max(0, min_len - total)
    return pre, pre + total


def frame(sig, noise, pad_len, min_len):
    pre, _ = layout(len(sig), pad_len, min_len)
    return np.concatenate((noise[:pre], noise[:pad_len], sig, noise[:pad_len]))


def component_error(got_c64, w):
    """max over samples and components of |got - exp(2 pi i w / 2^64)|"""
    ref = iq(w)
    g = np.asarray(got_c64).astype(np.complex128)
    return max(np.abs(g.real - ref.real).max(), np.abs(g.imag - ref.imag).max()) if len(g) else 0.0
