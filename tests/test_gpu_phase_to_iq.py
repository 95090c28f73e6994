"""``mod_phase_to_iq`` (pycusdr_amd/csrc/mod_kernels.hpp), the phase-word -> (cos, sin) routine the modulator, the channel and the
channeliser share, at chosen words.  Its documented bound is 4 * 2^-24 per component (``mm.BOUND``).

The probe is a channeliser plan whose output is the routine's result as values: taps h = [1.0], D = 2, one channel with a non-zero
word, cf32 input of ones.  Tap 0 is (h, 0), the accumulator becomes (1, +0), the rotation is fma(-+0, p.y, 1 * p.x) and
fma(0, p.x, 1 * p.y): y[m] == mod_phase_to_iq(w) with w = (0 - (m D) freq) mod 2^64.  The plan is set through the C ABI, so the
word in force is the one the test names."""
import ctypes as C

import numpy as np
import pytest

import modulator_model as mm
from pycusdr_amd import _lib

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1
D = 2


class Probe:
    def __init__(self, freq, max_out):
        self.lib = _lib.load()
        self.freq, self.max_out = int(freq), max_out
        self.h = C.c_void_p()
        assert self.lib.mfb_channelizer_create(C.byref(self.h), 0, 1, 1, D * max_out, max_out) == _lib.MFB_OK
        taps = np.ones(1, np.float32)
        words = np.array([self.freq], dtype=np.uint64)
        assert int(words[0]) == self.freq != 0                # the word in force
        assert self.lib.mfb_channelizer_set_plan(self.h, D, taps.ctypes.data, 1, words.ctypes.data, 1, 0, 1.0) == _lib.MFB_OK
        host, nbytes = C.c_void_p(), C.c_size_t()
        assert self.lib.mfb_channelizer_input_buffer(self.h, 0, C.byref(host), C.byref(nbytes)) == _lib.MFB_OK
        assert nbytes.value == 8 * D * max_out
        x = np.frombuffer((C.c_uint8 * nbytes.value).from_address(host.value), dtype=np.complex64)
        x[:] = 1.0 + 0.0j

    def run(self, out_base, nout):
        """(words as Python integers, outputs complex64)"""
        assert nout <= self.max_out
        P = _lib.ChannelizerParams(in_base=out_base * D, out_base=out_base, in_count=(nout - 1) * D + 1, out_count=nout, input=0, buffer=0)
        assert self.lib.mfb_channelizer_begin(self.h, C.byref(P)) == _lib.MFB_OK
        y = np.empty(nout, np.complex64)
        assert self.lib.mfb_channelizer_end(self.h, y.ctypes.data) == _lib.MFB_OK
        w = [(0 - (out_base + j) * D * self.freq) & MASK for j in range(nout)]
        return w, y

    def close(self):
        if self.h:
            self.lib.mfb_channelizer_destroy(self.h)
            self.h = C.c_void_p()


def errors(w, y):
    """per-component error of every sample against exp(2 pi i w / 2^64) in float64"""
    ref = mm.iq(np.array(w, dtype=np.uint64))
    g = y.astype(np.complex128)
    return np.maximum(np.abs(g.real - ref.real), np.abs(g.imag - ref.imag))


@pytest.fixture(scope='module')
def seam_probe():
    p = Probe((1 << 64) - (1 << 28), 192)                     # w = m * 2^29: one unit of the 32-bit octant fraction per output
    yield p
    p.close()


WORST_SEAM = {}


@pytest.mark.parametrize('k', range(1, 9))
def test_octant_seams(seam_probe, k):
    """192 consecutive fractions r = 0xFFFFFFA0 .. 0x5F across the boundary into octant k mod 8: the largest fractions of one
    octant, r = 0 of the next -- the mirrored 2^32 case for k = 1, 3, 5, 7, the word 0 that multiplies nothing for k = 8."""
    w, y = seam_probe.run(k * (1 << 32) - 96, 192)
    assert w == [((k << 61) + (j - 96) * (1 << 29)) & MASK for j in range(192)]
    assert [(v >> 29) & 0xFFFFFFFF for v in (w[0], w[95], w[96], w[191])] == [0xFFFFFFA0, 0xFFFFFFFF, 0, 0x5F]
    assert [v >> 61 for v in (w[95], w[96])] == [(k - 1) % 8, k % 8]
    e = errors(w, y)
    WORST_SEAM[k % 8] = float(e.max()) / 2.0 ** -24
    print(f'seam into octant {k % 8}: worst component error {WORST_SEAM[k % 8]:.3f} * 2^-24; so far {dict(sorted(WORST_SEAM.items()))}')
    assert e.max() <= mm.BOUND, (k, int(e.argmax()), e.max() / 2.0 ** -24)
    seam = y[96]
    if k % 2 == 0:                                            # a quarter turn: the polynomials at x = 0
        want = {0: (1.0, 0.0), 2: (0.0, 1.0), 4: (-1.0, 0.0), 6: (0.0, -1.0)}[k % 8]
        assert (float(seam.real), float(seam.imag)) == want, (k, seam)          # == : the sign of a zero is not pinned
    step = 2 * np.pi * 2.0 ** -35
    for nb in (y[95], y[97]):
        assert abs(float(nb.real) - float(seam.real)) <= 2 * mm.BOUND + step, (k, nb, seam)
        assert abs(float(nb.imag) - float(seam.imag)) <= 2 * mm.BOUND + step, (k, nb, seam)


def test_dense_sweep():
    """2^16 words 2 m * 0x9E3779B97F4A7C15 (golden-ratio steps: every octant, the low fraction bits all in use)."""
    freq, n = 0x9E3779B97F4A7C15, 1 << 16
    p = Probe(freq, n)
    try:
        w, y = p.run(0, n)
    finally:
        p.close()
    assert w[1] == (0 - 2 * freq) & MASK and w[0] == 0
    e = errors(w, y)
    octant = np.array([v >> 61 for v in w])
    per = [float(e[octant == o].max()) / 2.0 ** -24 for o in range(8)]
    assert all((octant == o).sum() > 7000 for o in range(8))
    print('dense sweep, worst component error per octant (2^-24): ' + '  '.join(f'{v:.3f}' for v in per) + f'; over all {max(per):.3f}')
    assert e.max() <= mm.BOUND, (int(e.argmax()), e.max() / 2.0 ** -24)
    assert np.abs(np.abs(y.astype(np.complex128)) - 1.0).max() <= 2 * mm.BOUND
