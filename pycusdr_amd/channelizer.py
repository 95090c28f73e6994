"""The channeliser in front of the banks: one wideband capture -- complex64, or the sc16 / sc8 integers a radio delivers -- becomes
K channels, each tuned to baseband, low-pass filtered with the plan's real taps and decimated by ``decim`` to the
``baud * samplesPerSym`` rate a bank is built for.  No reference counterpart: the reference takes one narrowband stream per radio
process (pyCuSDR.py:245-251).

With n the absolute position in the wideband stream, m the absolute position in a channel's output stream and ``freq_k`` the
channel's tuning word (uint64 turns * 2**64 per input sample, a negative frequency as the two's complement: the convention of
``modulator/phase.py`` and ``channel.signed_quantise``):

    phi_k(n) = n * freq_k                                                       (uint64, modulo 2**64)
    y_k[m]   = sum_{t < T} h[t] * x[m * D - t] * exp(-2 pi i phi_k(m * D - t) / 2**64)       x[n] = 0 for n < 0

``y_k[m]`` is a pure function of (h, D, freq_k, the T samples it reads, m): ``process`` gives the same samples whatever the spans it
is asked for in and whatever input window covers them, bit for bit.  ``backend='hip'`` is the mfb_channelizer_* handle of
include/mfbank.h (csrc/channelize_kernels.hpp has the rules); ``backend='host'`` is the model: exactly the sum above, mix first, in
float64 on exact uint64 words, rounded to complex64 at the end -- the yardstick for the device.

Rational resampling (``interp = U > 1``; mfb_channelizer_set_plan_rational, csrc/channelize_rational_kernels.hpp).  A plan holds an
interpolation ``U`` and a decimation ``D`` (1 <= U <= 32, 2 <= D <= 64, gcd(U, D) = 1, U < D: net rate reduction only), real taps
``h[0..T)`` given at the virtual rate ``U * fs`` (U <= T <= 1024) and the K words, still per INPUT sample:

    q(m) = (m D) div U        r(m) = (m D) mod U
    y_k[m] = sum over j >= 0 with r + jU < T of
             h[r + jU] x[q - j] exp(-2 pi i phi_k(q - j) / 2**64)       phi_k(n) = n freq_k mod 2**64,  x[n] = 0 for n < 0

the zero-stuff, filter, keep-every-D-th definition restricted to the products that are not zero.  The device computes it as
``exp(-2 pi i phi_k(q) / 2**64) * sum_j g_k[r + jU] x[q - j]`` with ``g_k[t] = h[t] exp(+2 pi i phi_k(t div U) / 2**64)``, exact
because phi_k is linear in integers.  One lane makes one output; the sum starts from (-0, -0); terms are added in the order
j = 0, 1, ...: for each tap the x.re terms, then the x.im terms; ``freq_k == 0`` uses h itself with one real multiply-add per
component and is not rotated; a rotation word of 0 multiplies nothing.  A branch runs its own ``ceil((T - r) / U)`` taps and no
padded ones.  ``y_k[m]`` stays a pure function of (h, U, D, freq_k, the samples it reads, m).  With ``U = 1`` the definition is the
one above, and ``Channelizer(...)`` without ``interp`` keeps running the integer kernel.  A call's outputs
``[out_base, out_base + out_count)`` read inputs ``[q(out_base) - (ceil(T / U) - 1), q(out_base + out_count - 1)]``, the uniform
bound, one sample generous for short branches.  ``factor_rate`` splits a ratio outside the limits into stages; a second stage is an
ordinary ``Channelizer`` with ``freqs_hz=[0.0]`` fed the first stage's ``device_output`` pointer.

Channels on a raster (``UniformChannelizer``; mfb_channelizer_create_uniform, csrc/channelize_uniform_kernels.hpp).  With every
centre a multiple of ``fs / M``, M a power of two, the words ``freq_k = k 2**64 / M`` are exact and the first definition collapses:

    y_k[m] = sum_{s < M} v_m[s] exp(+2 pi i k s / M)       v_m[s] = u_m[(s + m D) mod M]
    u_m[p] = sum over j with p + jM < T of h[p + jM] x[m D - p - jM]                      p = 0 .. M - 1

M branch sums with real taps, a circular shift and one M-point transform per output frame give all M bins: 2 T + 5 M log2 M flops
instead of 8 M T.  The yardstick stays the float64 model above on those words.

Resampling on the raster (``UniformChannelizer(..., interp=U)``; mfb_uniform_channelizer_set_plan_rational,
csrc/channelize_uniform_rational_kernels.hpp).  The rational definition collapses on those words in the same way, with ``q`` in the
place of ``m D`` and the frame's branch ``h[r + jU]`` in the place of the taps:

    y_k[m] = sum_{s < M} v_m[s] exp(+2 pi i k s / M)       v_m[s] = u_m[(s + q) mod M]
    u_m[p] = sum over i with r + (p + iM) U < T of h[r + (p + iM) U] x[q - p - iM]        p = 0 .. M - 1

1 <= U <= 32, U < D <= U M (the output rate does not fall below the bin spacing), ``ceil(T / U) <= 4096``.  The yardstick is the
rational model above on those words; per component the device is within ``(ceil(ceil(T / U) / M) + 3 log2 M + 2) 2**-24 S_m``.

The survey of the raster (``UniformChannelizer.set_survey`` / ``survey``; mfb_channelizer_set_survey,
csrc/channelize_survey_kernels.hpp): which bins hold a signal, and when, without writing any of them.  With ``y_k[m]`` the uniform
plan's complex64 output of bin k = 0 .. M - 1 and a cell length ``L = 2**l`` frames, 2 <= l <= 16:

    p_k[m]   = fl(fl(re * re) + fl(im * im))                     float32, not fused
    P[s][k]  = the balanced pairwise sum of p_k[s L .. s L + L)   at each level q[i] = fl(q[2 i] + q[2 i + 1])
    floor[s] = the rank-th smallest (0-based) of P[s][0 .. M)     default rank M / 4: on noise while < 3/4 of the raster is occupied
    mask     bit (s, k) is set iff P[s][k] > fl(threshold * floor[s]); uint32 [s][ceil(M / 32)], bit j of word w is bin 32 w + j

``pairwise_sum_f32``, ``cell_power``, ``cell_floor`` and ``cell_mask`` state these in numpy; the device gives the same bits from
its own ``y`` whatever the cut into calls, the input window, the output set, the selected bins and whether outputs are written.
``backend='host'`` applies them to the float64 model's outputs rounded to complex64.  ``bursts`` turns a mask into records per bin.
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np

from . import _lib
from ._handle import OutputStage
from .channel import signed_quantise
from .modulator import phase

_U = np.uint64
MAX_CHANNELS, MAX_DECIM, MAX_TAPS, MAX_IN, MAX_OUT = 16, 64, 1024, 1 << 24, 1 << 22
MAX_INTERP = 32
UNIFORM_BINS, UNIFORM_MAX_TAPS, UNIFORM_MAX_SET = (8, 16, 32, 64, 128, 256), 4096, 1 << 26
FORMATS = {'cf32': 0, 'sc16': 1, 'sc8': 2}           # MFB_SAMPLES_* of include/mfbank.h
_RAW = {'sc16': np.int16, 'sc8': np.int8}
INPUT_PINNED0, INPUT_PINNED1, INPUT_DEVICE = 0, 1, 2


def design_taps(decim, taps_per_phase=16, beta=8.0, cutoff=0.4, interp=1):
    """A Kaiser-windowed sinc low-pass for a decimation by ``decim``: ``T = decim * taps_per_phase + 1`` taps, float32, cutoff
    (the -6 dB point) at ``cutoff / decim`` cycles per input sample, unit gain at DC.  The taps are symmetric: the group delay is
    ``(T - 1) / 2`` input samples, ``taps_per_phase / 2`` output samples.  With ``interp = U > 1`` the same taps stand at the
    virtual rate ``U * fs`` of a resampling by U / decim: cutoff at ``cutoff / decim`` cycles per virtual sample, that is ``cutoff``
    cycles per output sample; they sum to U, so every branch has about unit gain and the pass-band gain is 1; the group delay is
    ``(T - 1) / (2 U)`` input samples.  For a ``UniformChannelizer`` of M bins ``design_taps(decim)`` is the right prototype as it
    is: every bin's pass band is ``0.4 / decim`` cycles per input sample to either side of its centre, so adjacent bins, ``1 / M``
    apart, overlap as the taps dictate when ``decim < 0.8 M`` and are disjoint to -6 dB from there up to critical sampling."""
    decim, taps_per_phase, interp = int(decim), int(taps_per_phase), int(interp)
    if decim < 1 or taps_per_phase < 1 or interp < 1 or not 0 < cutoff <= 0.5:
        raise ValueError('decim >= 1, taps_per_phase >= 1, interp >= 1, 0 < cutoff <= 0.5')
    T = decim * taps_per_phase + 1
    fc = cutoff / decim
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * n) * np.kaiser(T, beta)
    if interp == 1:
        return (h / h.sum()).astype(np.float32)
    return (h * (interp / h.sum())).astype(np.float32)


def check_plan(decim, taps, words, sample_format, sample_scale, interp=1):
    """The checks of mfb_channelizer_set_plan and, for ``interp``, of mfb_channelizer_set_plan_rational, as ValueError: (decim,
    taps float32, words uint64, scale)."""
    decim, interp = int(decim), int(interp)
    taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    if not 2 <= decim <= MAX_DECIM:
        raise ValueError(f'2 <= decim <= {MAX_DECIM}')
    if not 1 <= len(taps) <= MAX_TAPS or not np.all(np.isfinite(taps)):
        raise ValueError(f'1 .. {MAX_TAPS} finite taps')
    if not 1 <= len(words) <= MAX_CHANNELS:
        raise ValueError(f'1 .. {MAX_CHANNELS} channels')
    if not 1 <= interp <= MAX_INTERP:
        raise ValueError(f'1 <= interp <= {MAX_INTERP}')
    if interp >= decim or math.gcd(interp, decim) != 1:
        raise ValueError('interp < decim, and the two have no common factor')
    if len(taps) < interp:
        raise ValueError('at least interp taps: every branch has one')
    if sample_format not in FORMATS:
        raise ValueError(f'sample_format is one of {sorted(FORMATS)}')
    scale = float(sample_scale)
    if sample_format != 'cf32':
        m, e = np.frexp(np.float32(scale))
        if not (np.isfinite(scale) and scale > 0 and m == 0.5 and -100 < e < 100):
            raise ValueError('sample_scale is a power of two')
    return decim, taps, words, scale


def factor_rate(fs_in, fs_out):
    """The stages ``[(U_1, D_1), ...]`` that take ``fs_in`` to ``fs_out``: each within a plan's limits (1 <= U <= 32, 2 <= D <= 64,
    U < D, no common factor; an integer stage is ``(1, D)``), the product of the U_i / D_i exactly ``fs_out / fs_in`` (taken with
    ``fractions.Fraction``; the U_i multiply to its numerator and the D_i to its denominator).  The fewest stages; among lists of
    equal length the largest rate reduction goes to the first stage, then to the second, and so on.  ValueError where no such list
    exists: a ratio >= 1, a prime factor of the denominator above 64 or of the numerator above 32."""
    ratio = Fraction(fs_out) / Fraction(fs_in)
    u, d = ratio.numerator, ratio.denominator
    if not 0 < ratio < 1:
        raise ValueError('0 < fs_out < fs_in: net rate reduction only')

    def stages_of(u, d):
        # (U, D) is coprime whenever U | u and D | d, because u / d is in lowest terms
        return [(a, b) for b in range(2, MAX_DECIM + 1) if d % b == 0 for a in range(1, min(b, MAX_INTERP + 1)) if u % a == 0]

    @functools.lru_cache(maxsize=None)
    def split(u, d, n):
        """The best list of exactly n stages for u / d, or None."""
        if n == 1:
            return [(u, d)] if u <= MAX_INTERP and 2 <= d <= MAX_DECIM and u < d else None
        for a, b in sorted(stages_of(u, d), key=lambda s: Fraction(s[0], s[1])):
            rest = split(u // a, d // b, n - 1)
            if rest is not None:
                return [(a, b)] + rest
        return None

    for n in range(1, d.bit_length() + 1):                  # every stage at least halves the denominator
        got = split(u, d, n)
        if got is not None:
            return got
    raise ValueError(f'{u}/{d} is no product of stages U / D with U <= {MAX_INTERP}, D <= {MAX_DECIM}, U < D')


def samples_to_c64(samples, sample_format, scale):
    """What the device makes of raw input: complex64 as it is; int16 / int8 I, Q pairs as ``raw.astype(float32) * scale``."""
    if sample_format == 'cf32':
        return np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
    raw = np.ascontiguousarray(samples, dtype=_RAW[sample_format]).reshape(-1, 2)
    f = raw.astype(np.float32) * np.float32(scale)
    return (f[:, 0] + 1j * f[:, 1]).astype(np.complex64)


def _model_integer(taps, words, D, in_base, x, out_base, out_count):
    """The integer-decimation definition in float64 on exact uint64 words, mix first: (y complex128 [K, out_count], S float64
    [out_count]).  ``x`` complex128, the input from ``in_base`` on.  ``Channelizer.model`` and ``UniformChannelizer.model``."""
    T = len(taps)
    first = out_base * D - (T - 1)                          # may be negative: those positions read as zero
    span = (out_count - 1) * D + T
    lo = max(first, 0)
    seg = np.zeros(span, dtype=np.complex128)
    seg[lo - first:] = x[lo - in_base:first + span - in_base]
    n = np.arange(lo, first + span, dtype=np.int64).astype(np.uint64)
    hrev = taps.astype(np.float64)[::-1]
    win = np.lib.stride_tricks.sliding_window_view
    y = np.empty((len(words), out_count), dtype=np.complex128)
    for k, f in enumerate(words):
        z = seg
        if f != 0:
            with np.errstate(over='ignore'):
                w = _U(0) - n * _U(f)                       # -phi_k(n), exact
            z = seg.copy()
            z[lo - first:] = np.where(w == 0, seg[lo - first:], seg[lo - first:] * phase.words_to_iq(w))
        y[k] = win(z, T)[::D] @ hrev                       # row j: z[j D .. j D + T - 1], tap t at j D + T - 1 - t
    S = win(np.abs(seg), T)[::D] @ np.abs(hrev)
    return y, S


class Channelizer(OutputStage):
    PREFIX = 'mfb_channelizer'

    def __init__(self, fs, decim, taps, freqs_hz, sample_format='cf32', sample_scale=1.0, backend='hip', device=0, max_in=1 << 20,
                 max_out=None, interp=1, force_rational=False):
        """``interp = U``: resample by U / decim (the module docstring); 1 takes the integer kernel, unless ``force_rational``
        (the tests' seam) sends that plan through the rational kernel too."""
        self._check_backend(fs, backend, device)
        freqs = np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
        if not np.all(np.abs(freqs) <= self.fs / 2):
            raise ValueError('|freq| <= fs / 2')
        self.freqs_hz = freqs
        self.decim, self.taps, self.words, self.scale = check_plan(decim, taps, signed_quantise(phase.TWO_PI * freqs / self.fs),
                                                                   sample_format, sample_scale, interp)
        self.interp = int(interp)
        self.rational = self.interp > 1 or bool(force_rational)
        self.sample_format, self.T, self.K = sample_format, len(self.taps), len(self.words)
        self._init_tail(max_in, max_out)
        if backend == 'hip':
            _lib.check(self.lib.mfb_channelizer_create(C.byref(self.h), device, self.K, self.T, self.max_in, self.max_out),
                       'mfb_channelizer_create')
            plan = (self.decim, self.taps.ctypes.data, self.T, self.words.ctypes.data, self.K, FORMATS[sample_format], self.scale)
            if self.rational:
                self._call('mfb_channelizer_set_plan_rational', self.interp, *plan)
            else:
                self._call('mfb_channelizer_set_plan', *plan)

    def _check_backend(self, fs, backend, device):
        if backend not in ('hip', 'host'):
            raise ValueError("backend is 'hip' or 'host'")
        self.fs, self.backend, self.device = float(fs), backend, device

    def _init_tail(self, max_in, max_out, max_set=None):
        """What every constructor ends with, once ``interp``, ``decim``, ``T`` and ``K`` stand: the longest branch, the sizes of a
        call with their limits (``max_set``: complex64 per output set), the buffers' flip state, an empty handle and the library."""
        self.Tb = -(-self.T // self.interp)                   # taps of the longest branch
        self.max_in = int(max_in)
        self.max_out = int(max_out) if max_out is not None else max(1, -(-self.max_in * self.interp // self.decim))
        if not (1 <= self.max_in <= MAX_IN and 1 <= self.max_out <= MAX_OUT):
            raise ValueError('1 <= max_in <= 2**24, 1 <= max_out <= 2**22')
        if max_set is not None and self.K * self.max_out > max_set:
            raise ValueError('selected bins * max_out <= 2**26 samples per output set')
        self._buffer, self._which, self._pinned = 1, 1, [None, None]
        self.h = C.c_void_p()
        if self.backend == 'hip':
            self.lib = _lib.load()

    def close(self):
        if self.h:
            self._pinned = [None, None]                       # (views of page-locked memory that goes with the handle)
        super().close()

    def info(self):
        """(outputs per workgroup, tap capacity) of the plan in force (hip)."""
        a, b = C.c_int(), C.c_int()
        self._call('mfb_channelizer_info', C.byref(a), C.byref(b))
        return a.value, b.value

    def elapsed_ms(self):
        ms = C.c_float()
        self._call('mfb_channelizer_elapsed_ms', C.byref(ms))
        return ms.value

    def needed_input(self, out_base, out_count):
        """(in_base, in_count): the input positions that outputs out_base .. out_base + out_count read, clipped at 0: from
        ``q(out_base) - (ceil(T / U) - 1)`` to ``q(out_base + out_count - 1)`` with ``q(m) = (m D) div U``."""
        out_base, out_count = int(out_base), int(out_count)
        if out_base < 0 or out_count < 1:
            raise ValueError('out_base >= 0, out_count >= 1')
        first = max(0, out_base * self.decim // self.interp - (self.Tb - 1))
        last = (out_base + out_count - 1) * self.decim // self.interp
        return first, last - first + 1

    def _checked(self, in_base, in_count, out_base, out_count):
        if in_base < 0 or out_base < 0 or in_count < 1 or out_count < 1:
            raise ValueError('bases >= 0, counts >= 1')
        if in_base >= 1 << 62 or out_base * self.decim >= 1 << 62:
            raise ValueError('in_base, out_base * decim < 2**62')
        if in_count > self.max_in or out_count > self.max_out:
            raise ValueError(f'at most max_in = {self.max_in} inputs and max_out = {self.max_out} outputs per call')
        first, n = self.needed_input(out_base, out_count)
        if first < in_base or first + n > in_base + in_count:
            raise ValueError(f'outputs {out_base} .. {out_base + out_count} read inputs {first} .. {first + n}: '
                             f'not inside {in_base} .. {in_base + in_count}')

    def input_buffer(self, which):
        """The page-locked staging buffer ``which`` (0 or 1) as a numpy array of the plan's sample format: complex64 [max_in], or
        int16 / int8 [max_in, 2]."""
        if self._pinned[which] is None:
            ptr, nbytes = C.c_void_p(), C.c_size_t()
            self._call('mfb_channelizer_input_buffer', which, C.byref(ptr), C.byref(nbytes))
            raw = (C.c_uint8 * nbytes.value).from_address(ptr.value)
            if self.sample_format == 'cf32':
                self._pinned[which] = np.frombuffer(raw, dtype=np.complex64)
            else:
                self._pinned[which] = np.frombuffer(raw, dtype=_RAW[self.sample_format]).reshape(-1, 2)
        return self._pinned[which]

    def process(self, in_base, samples, out_base, out_count, copy=True, buffer=None):
        """Outputs out_base .. out_base + out_count of every channel from the input that begins at absolute position ``in_base``:
        host samples of the plan's format (complex, or int16 / int8 [n, 2]), or -- hip -- device memory as ``(device_ptr, count)``
        (a bare pointer stands for exactly what ``needed_input`` asks for from ``in_base`` on).  ``copy``: complex64
        [K, out_count]; not ``copy`` (hip): the outputs stay in the handle's output set ``buffer`` (default: the one not written
        last), ask ``device_output`` for them."""
        self.begin(in_base, samples, out_base, out_count, buffer)
        return self.end(copy)

    def _intake(self, in_base, samples, out_base, out_count):
        """``samples`` as ``process`` takes them, checked against the span: (on_device, device pointer or host array of the plan's
        format, in_count)."""
        on_device = isinstance(samples, (int, tuple))
        if on_device:
            if self.backend != 'hip':
                raise ValueError("device memory is an input of the 'hip' back end")
            if isinstance(samples, tuple):
                x, in_count = int(samples[0]), int(samples[1])
            else:
                first, n = self.needed_input(out_base, max(out_count, 1))
                x, in_count = int(samples), first + n - in_base
        else:
            if self.sample_format == 'cf32':
                x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
            else:
                x = np.ascontiguousarray(samples, dtype=_RAW[self.sample_format]).reshape(-1, 2)
            in_count = len(x)
        self._checked(in_base, in_count, out_base, out_count)
        return on_device, x, in_count

    def _params(self, on_device, x, in_base, in_count, out_base, out_count, buffer):
        """The ``ChannelizerParams`` of a device call (``_count`` is the caller's to set once the call is begun): flips the output set unless ``buffer`` names one, and copies host samples
        into the page-locked buffer that the call before did not use."""
        self._buffer = (self._buffer ^ 1) if buffer is None else int(buffer)
        P = _lib.ChannelizerParams(in_base=in_base, out_base=out_base, in_count=in_count, out_count=out_count, buffer=self._buffer)
        if on_device:
            P.input, P.device_input = INPUT_DEVICE, x
        else:
            self._which ^= 1
            self.input_buffer(self._which)[:in_count] = x
            P.input = INPUT_PINNED1 if self._which else INPUT_PINNED0
        return P

    def begin(self, in_base, samples, out_base, out_count, buffer=None):
        in_base, out_base, out_count = int(in_base), int(out_base), int(out_count)
        on_device, x, in_count = self._intake(in_base, samples, out_base, out_count)
        if self.backend == 'host':
            self._host = self.model(in_base, x, out_base, out_count)[0].astype(np.complex64)
            return
        P = self._params(on_device, x, in_base, in_count, out_base, out_count, buffer)
        self._call('mfb_channelizer_begin', C.byref(P))
        self._count = out_count

    def end(self, copy=True):
        return self._end(copy, self.K)                        # complex64 [K, out_count]; not ``copy``: None

    def device_output(self, buffer, k):
        """(device_ptr, count) of channel ``k`` in output set ``buffer``."""
        return self._device_output(buffer, k)

    def model(self, in_base, samples, out_base, out_count):
        """The definition in float64, mix first, before rounding: (y complex128 [K, out_count], S float64 [out_count]) with
        ``S[m] = sum_t |h[t]| |x[m D - t]|`` (``sum_j |h[r + jU]| |x[q - j]|`` when resampling), the scale of the device's error
        bound."""
        in_base, out_base, out_count = int(in_base), int(out_base), int(out_count)
        x = samples_to_c64(samples, self.sample_format, self.scale).astype(np.complex128)
        self._checked(in_base, len(x), out_base, out_count)
        if self.interp > 1:
            return self._model_rational(in_base, x, out_base, out_count)
        return _model_integer(self.taps, self.words, self.decim, in_base, x, out_base, out_count)

    def _model_rational(self, in_base, x, out_base, out_count):
        """``model`` for U > 1: the sum of the definition, tap by tap, over the mixed stream."""
        U, D, T = self.interp, self.decim, self.T
        md = (out_base + np.arange(out_count, dtype=np.int64)) * D
        q, r = md // U, md % U
        first = int(q[0]) - (self.Tb - 1)                   # may be negative: those positions read as zero
        lo = max(first, 0)
        seg = np.zeros(int(q[-1]) - first + 1, dtype=np.complex128)
        seg[lo - first:] = x[lo - in_base:int(q[-1]) + 1 - in_base]
        n = np.arange(lo, int(q[-1]) + 1, dtype=np.int64).astype(np.uint64)
        z = np.empty((self.K, len(seg)), dtype=np.complex128)
        for k, f in enumerate(self.words):
            z[k] = seg
            if f != 0:
                with np.errstate(over='ignore'):
                    w = _U(0) - n * _U(f)                   # -phi_k(n), exact
                z[k, lo - first:] = np.where(w == 0, seg[lo - first:], seg[lo - first:] * phase.words_to_iq(w))
        h = np.r_[self.taps.astype(np.float64), np.zeros(U)]      # (a branch's taps beyond T count as absent: they add exact zeros)
        mag = np.abs(seg)
        at = q - first
        y = np.zeros((self.K, out_count), dtype=np.complex128)
        S = np.zeros(out_count, dtype=np.float64)
        for j in range(self.Tb):
            t = np.minimum(r + j * U, T)
            y += h[t] * z[:, at - j]
            S += np.abs(h[t]) * mag[at - j]
        return y, S


def check_plan_uniform(nbins, decim, taps, bins, sample_format, sample_scale, interp=1):
    """The checks of mfb_channelizer_create_uniform and mfb_channelizer_set_plan_uniform and, for ``interp``, of
    mfb_uniform_channelizer_set_plan_rational, as ValueError: (M, decim, taps float32, bins int32 in [0, M), scale).  ``bins``:
    indices -M/2 <= b < M, taken modulo M; None: all M in index order."""
    M, decim, interp = int(nbins), int(decim), int(interp)
    if M not in UNIFORM_BINS:
        raise ValueError(f'nbins is one of {UNIFORM_BINS}')
    if not 1 <= interp <= MAX_INTERP:
        raise ValueError(f'1 <= interp <= {MAX_INTERP}')
    if not 2 <= decim <= interp * M:
        raise ValueError('2 <= decim <= interp * nbins: the output rate does not fall below the bin spacing')
    if interp >= decim or math.gcd(interp, decim) != 1:
        raise ValueError('interp < decim, and the two have no common factor')
    taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if not 1 <= -(-len(taps) // interp) <= UNIFORM_MAX_TAPS or not np.all(np.isfinite(taps)):
        raise ValueError(f'1 .. {UNIFORM_MAX_TAPS} finite taps per branch (interp * {UNIFORM_MAX_TAPS} in all)')
    if len(taps) < interp:
        raise ValueError('at least interp taps: every branch has one')
    b = np.arange(M, dtype=np.int64) if bins is None else np.atleast_1d(np.asarray(bins)).reshape(-1)
    if b.dtype.kind not in 'iu':
        raise ValueError('bins are integers')
    b = b.astype(np.int64)
    if not 1 <= len(b) <= M:
        raise ValueError('1 .. nbins selected bins')
    if np.any(b < -(M // 2)) or np.any(b >= M):
        raise ValueError('-nbins / 2 <= bin < nbins')
    b = (b % M).astype(np.int32)
    if len(np.unique(b)) != len(b):
        raise ValueError('a bin is selected twice')
    if sample_format not in FORMATS:
        raise ValueError(f'sample_format is one of {sorted(FORMATS)}')
    scale = float(sample_scale)
    if sample_format != 'cf32':
        m, e = np.frexp(np.float32(scale))
        if not (np.isfinite(scale) and scale > 0 and m == 0.5 and -100 < e < 100):
            raise ValueError('sample_scale is a power of two')
    return M, decim, taps, b, scale


def uniform_rate(fs_in, fs_out, nbins):
    """(U, D), the ratio ``fs_out / fs_in`` in lowest terms (taken with ``fractions.Fraction``), for a
    ``UniformChannelizer(fs_in, nbins, D, design_taps(D, interp=U), interp=U)``: ``uniform_rate(2.4e6, 153600, 64) == (8, 125)``.
    ValueError where one plan cannot do it: nbins outside the set, a ratio >= 1, U > 32, or D > U * nbins (an output rate below the
    bin spacing)."""
    M = int(nbins)
    if M not in UNIFORM_BINS:
        raise ValueError(f'nbins is one of {UNIFORM_BINS}')
    ratio = Fraction(fs_out) / Fraction(fs_in)
    if not 0 < ratio < 1:
        raise ValueError('0 < fs_out < fs_in: net rate reduction only')
    U, D = ratio.numerator, ratio.denominator
    if U > MAX_INTERP:
        raise ValueError(f'{U}/{D}: interp <= {MAX_INTERP}')
    if D > U * M:
        raise ValueError(f'{U}/{D}: decim <= interp * nbins = {U * M}, the output rate does not fall below the bin spacing')
    return U, D


class UniformChannelizer(Channelizer):
    """The channels of a raster: bin b of ``nbins = M`` (8 .. 256, a power of two) sits at ``b * fs / M``, is filtered with the real
    ``taps`` and decimated by ``decim`` (2 <= D <= M; D need not divide M, critical sampling is D = M).  The definition is
    ``Channelizer``'s with the exact words ``(b << 64) // M``; the device computes all M bins of an output frame with one M-point
    transform over M branch sums (csrc/channelize_uniform_kernels.hpp, mfb_channelizer_create_uniform) and writes the selected
    ``bins`` -- indices, signed or unsigned: -M/2 <= b < M, taken modulo M; None: all M in index order --, row i of the output
    being ``bins[i]``.  ``design_taps(decim)`` is the prototype for it.  Everything else is ``Channelizer``'s surface: ``K`` is the
    number of selected bins, ``interp`` is 1, ``info()`` gives (frames per workgroup, tap capacity); ``backend='host'`` and
    ``model`` are the same float64 arithmetic on the exact words.  ``ChannelizerSource`` and ``ChannelWide`` take it as it is.

    ``interp = U > 1`` resamples every bin by U / decim instead (the module docstring; mfb_uniform_channelizer_set_plan_rational,
    csrc/channelize_uniform_rational_kernels.hpp): 1 <= U <= 32, U < D <= U M, no common factor, taps at the virtual rate ``U fs``
    with U <= T and ``ceil(T / U) <= 4096``; ``design_taps(decim, interp=U)`` is the prototype, ``uniform_rate`` gives (U, D) for
    two rates.  ``interp`` and ``rational`` are then set as ``Channelizer`` sets them, so ``needed_input``, ``model``,
    ``backend='host'`` and ``ChannelizerSource`` are the rational ones; ``info()`` gives the frames per workgroup of that plan and
    the taps of the longest branch; ``set_survey`` raises."""

    def __init__(self, fs, nbins, decim, taps, bins=None, sample_format='cf32', sample_scale=1.0, backend='hip', device=0, max_in=1 << 20,
                 max_out=None, interp=1, force_rational=False):
        """``interp = U``: resample every bin by U / decim (the class docstring); 1 takes the integer kernel, unless
        ``force_rational`` (the tests' seam) sends that plan through the rational kernel too."""
        self._check_backend(fs, backend, device)
        self.nbins, self.decim, self.taps, self.bins, self.scale = check_plan_uniform(nbins, decim, taps, bins, sample_format, sample_scale,
                                                                                      interp)
        # exact: M is a power of two.  (The float route signed_quantise(2 pi f / fs) rounds some of them differently from M = 64 on.)
        self.words = np.array([(int(b) << 64) // self.nbins for b in self.bins], dtype=np.uint64)
        self.interp = int(interp)
        self.rational = self.interp > 1 or bool(force_rational)
        self.sample_format, self.T, self.K = sample_format, len(self.taps), len(self.bins)
        self._init_tail(max_in, max_out, UNIFORM_MAX_SET)
        if backend == 'hip':
            # the handle's tap capacity: the taps of a frame -- T, or the longest branch of a rational plan
            _lib.check(self.lib.mfb_channelizer_create_uniform(C.byref(self.h), device, self.nbins, self.K, self.Tb, self.max_in, self.max_out),
                       'mfb_channelizer_create_uniform')
            plan = (self.decim, self.taps.ctypes.data, self.T, self.bins.ctypes.data, self.K, FORMATS[sample_format], self.scale)
            if self.rational:
                self._call('mfb_uniform_channelizer_set_plan_rational', self.interp, *plan)
            else:
                self._call('mfb_channelizer_set_plan_uniform', *plan)

    @property
    def freqs_hz(self):
        """The selected bins' centres, the upper half of the raster as negative frequencies: ``b * fs / M`` for b < M / 2."""
        b = self.bins.astype(np.int64)
        return np.where(b >= self.nbins // 2, b - self.nbins, b) * (self.fs / self.nbins)

    # ---- the survey of the raster (the section of the module docstring; mfb_channelizer_set_survey)
    _survey = None                                           # (cell_frames, rank, threshold)

    def set_survey(self, cell_frames, rank=None, threshold=4.0):
        """The cell length L (a power of two, 4 .. 65536, at most ``max_out``), the floor's rank (default M / 4) and the mask's
        threshold (finite, >= 1) of the ``survey`` calls to come.  ``cell_frames = 0`` turns the survey off.  The survey is a matter
        of integer plans: ValueError under a rational one (``interp > 1`` or ``force_rational``)."""
        if self.rational:
            raise ValueError('the survey is not available under a rational plan')
        L = int(cell_frames)
        if L == 0:
            self._survey = None
            if self.backend == 'hip':
                self._call('mfb_channelizer_set_survey', 0, 0, 1.0)
            return
        rank = self.nbins // 4 if rank is None else int(rank)
        threshold = float(np.float32(threshold))
        if L & (L - 1) or not SURVEY_MIN_CELL <= L <= SURVEY_MAX_CELL:
            raise ValueError(f'cell_frames is a power of two, {SURVEY_MIN_CELL} .. {SURVEY_MAX_CELL}')
        if L > self.max_out:
            raise ValueError(f'a cell of {L} frames is longer than max_out = {self.max_out}')
        if not 0 <= rank < self.nbins:
            raise ValueError('0 <= rank < nbins')
        if not (np.isfinite(threshold) and threshold >= 1.0):
            raise ValueError('threshold is finite and >= 1')
        if self.backend == 'hip':
            self._call('mfb_channelizer_set_survey', L, rank, threshold)
        self._survey = (L, rank, threshold)

    def survey_info(self):
        """(frames per workgroup of a survey call, cell_frames, rank, threshold) on the device; cell_frames 0: no survey is set.
        Cells shorter than the first are summed inside a workgroup, longer ones across workgroups."""
        L, F, r, t = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        self._call('mfb_channelizer_survey_info', C.byref(L), C.byref(F), C.byref(r), C.byref(t))
        return F.value, L.value, r.value, t.value

    def needed_input_cells(self, first_cell, ncells):
        """(in_base, in_count): the input positions that the cells first_cell .. first_cell + ncells read, clipped at 0."""
        if self._survey is None:
            raise ValueError('no survey is set: set_survey first')
        L = self._survey[0]
        if int(first_cell) < 0 or int(ncells) < 1:
            raise ValueError('first_cell >= 0, ncells >= 1')
        return self.needed_input(int(first_cell) * L, int(ncells) * L)

    def survey(self, in_base, samples, first_cell, ncells, write=False, buffer=None, copy=True):
        """The cells first_cell .. first_cell + ncells of all M bins, from input given as to ``process``: a ``SurveyResult``.
        ``write``: the call also makes the outputs ``first_cell * L .. (first_cell + ncells) * L`` of the selected bins, exactly as
        ``process`` does, and returns ``(result, outputs)`` with outputs complex64 [K, ncells * L]; they also stand in output set
        ``buffer`` (hip); not ``copy`` (hip): they stay there alone, ask ``device_output`` for them, and outputs is None.  Without
        ``write`` no bin is written and that output set counts as never written."""
        if self._survey is None:
            raise ValueError('no survey is set: set_survey first')
        L, rank, threshold = self._survey
        in_base, first_cell, ncells = int(in_base), int(first_cell), int(ncells)
        if first_cell < 0 or ncells < 1:
            raise ValueError('first_cell >= 0, ncells >= 1')
        out_base, out_count = first_cell * L, ncells * L
        if self.nbins * out_count > UNIFORM_MAX_SET or self.nbins * ncells > SURVEY_MAX_TABLE:
            raise ValueError('nbins * frames <= 2**26 and nbins * cells <= 2**22 per survey call')
        on_device, x, in_count = self._intake(in_base, samples, out_base, out_count)
        if self.backend == 'host':
            xc = samples_to_c64(x, self.sample_format, self.scale).astype(np.complex128)
            every = np.array([(b << 64) // self.nbins for b in range(self.nbins)], dtype=np.uint64)
            y = _model_integer(self.taps, every, self.decim, in_base, xc, out_base, out_count)[0].astype(np.complex64)
            power = cell_power(y, L)
            floor = cell_floor(power, rank)
            res = SurveyResult(power, floor, cell_mask(power, floor, threshold), first_cell, L)
            return (res, y[self.bins]) if write else res
        P = self._params(on_device, x, in_base, in_count, out_base, out_count, buffer)
        self._call('mfb_channelizer_survey_begin', C.byref(P), 1 if write else 0)
        self._count = out_count
        power = np.empty((ncells, self.nbins), dtype=np.float32)
        floor = np.empty(ncells, dtype=np.float32)
        mask = np.empty((ncells, -(-self.nbins // 32)), dtype=np.uint32)
        out = np.empty((self.K, out_count), dtype=np.complex64) if write and copy else None
        self._call('mfb_channelizer_survey_end', out.ctypes.data if out is not None else None, power.ctypes.data, floor.ctypes.data, mask.ctypes.data)
        res = SurveyResult(power, floor, mask, first_cell, L)
        return (res, out) if write else res


SURVEY_MIN_CELL, SURVEY_MAX_CELL, SURVEY_MAX_TABLE = 4, 1 << 16, 1 << 22


def pairwise_sum_f32(p):
    """The balanced pairwise sum in float32 along the last axis, whose length is a power of two: at each level
    ``q[i] = fl(q[2 i] + q[2 i + 1])``.  Any aligned power-of-two run of the axis is a subtree."""
    q = np.ascontiguousarray(p, dtype=np.float32)
    n = q.shape[-1]
    if n < 1 or n & (n - 1):
        raise ValueError('the length of the last axis is a power of two')
    while q.shape[-1] > 1:
        q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def cell_power(y, cell_frames):
    """``P[s][k]`` float32 [ncells][M] of outputs ``y`` complex64 [M][ncells * L] whose first position is a multiple of L: the
    pairwise sum over every cell of ``p = fl(fl(re re) + fl(im im))``, each operation rounded to float32 on its own."""
    y = np.ascontiguousarray(y, dtype=np.complex64)
    L = int(cell_frames)
    if y.ndim != 2 or L < 1 or y.shape[1] % L:
        raise ValueError('y is [M][ncells * cell_frames]')
    re, im = y.real.astype(np.float32), y.imag.astype(np.float32)
    p = (re * re) + (im * im)
    return np.ascontiguousarray(pairwise_sum_f32(p.reshape(y.shape[0], -1, L)).T)


def cell_floor(power, rank):
    """``floor[s]``: the ``rank``-th smallest (0-based) of the M values of every cell."""
    power = np.asarray(power, dtype=np.float32)
    if not 0 <= int(rank) < power.shape[1]:
        raise ValueError('0 <= rank < M')
    return np.ascontiguousarray(np.sort(power, axis=1)[:, int(rank)])


def cell_mask(power, floor, threshold):
    """uint32 [ncells][ceil(M / 32)]: bit j of word w is set iff ``P[s][32 w + j] > fl(threshold * floor[s])``; unused bits zero."""
    power = np.asarray(power, dtype=np.float32)
    level = np.float32(threshold) * np.asarray(floor, dtype=np.float32)
    ncells, M = power.shape
    occ = np.zeros((ncells, -(-M // 32) * 32), dtype=bool)
    occ[:, :M] = power > level[:, None]
    return (occ.reshape(ncells, -1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)


def unpack_mask(mask, nbins):
    """bool [ncells][M] of the packed words."""
    mask = np.asarray(mask, dtype=np.uint32)
    bits = (mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(mask.shape[0], -1)[:, :nbins].astype(bool)


BURST = np.dtype([('bin', np.int32), ('first_cell', np.int64), ('last_cell', np.int64), ('peak_power', np.float32),
                  ('mean_power', np.float32)])


def bursts(mask, power, hang=0, min_cells=1, first_cell=0):
    """Runs of set cells per bin, host-only: runs separated by at most ``hang`` clear cells are merged, then runs shorter than
    ``min_cells`` (first to last cell, bridged cells included) are dropped.  Records of dtype ``BURST`` -- (bin, first_cell,
    last_cell, peak_power, mean_power), the cells counted from ``first_cell``, peak and mean over all cells from first to last, the
    mean in float64 rounded to float32 -- sorted by (first_cell, bin)."""
    power = np.asarray(power, dtype=np.float32)
    occ = unpack_mask(mask, power.shape[1])
    hang, min_cells = int(hang), int(min_cells)
    if hang < 0 or min_cells < 1:
        raise ValueError('hang >= 0, min_cells >= 1')
    found = []
    for k in range(occ.shape[1]):
        on = np.flatnonzero(occ[:, k])
        if not len(on):
            continue
        cut = np.flatnonzero(np.diff(on) > hang + 1)         # a gap of more than `hang` clear cells ends a run
        for a, b in zip(np.r_[on[0], on[cut + 1]], np.r_[on[cut], on[-1]]):
            if b - a + 1 >= min_cells:
                seg = power[a:b + 1, k]
                found.append((k, first_cell + a, first_cell + b, seg.max(), np.float32(seg.astype(np.float64).mean())))
    found.sort(key=lambda r: (r[1], r[0]))
    return np.array(found, dtype=BURST)


class SurveyResult:
    """``power`` float32 [ncells][M], ``floor`` float32 [ncells], ``mask`` uint32 [ncells][ceil(M / 32)] of the cells
    ``first_cell .. first_cell + ncells`` of ``cell_frames`` frames each, bins in natural order."""

    def __init__(self, power, floor, mask, first_cell, cell_frames):
        self.power, self.floor, self.mask, self.first_cell, self.cell_frames = power, floor, mask, int(first_cell), int(cell_frames)

    def occupied(self):
        """bool [ncells][M]: the mask unpacked."""
        return unpack_mask(self.mask, self.power.shape[1])

    def bursts(self, hang=0, min_cells=1):
        return bursts(self.mask, self.power, hang, min_cells, self.first_cell)


class ChannelWide:
    """A ``Channel`` as the wideband capture of a ``ChannelizerSource``: ``render(in_base, in_count)`` renders that span of the
    channel's stream on the device and returns its device pointer."""

    def __init__(self, channel, frames=(), sigma=0.0, mute_before=0, adc=None):
        from .channel import check_frames, pack_frames
        if channel.backend != 'hip':
            raise ValueError("the wideband capture is rendered with the 'hip' back end")
        self.channel, self.sigma, self.mute_before, self.adc = channel, sigma, int(mute_before), adc
        frames = list(frames)
        check_frames(frames, channel.source_len)
        self._starts = np.array([f.start for f in frames], dtype=np.int64)
        self._ends = np.array([f.start + f.length for f in frames], dtype=np.int64)
        self._packed = pack_frames(frames)

    def render(self, in_base, in_count):
        lo = int(np.searchsorted(self._ends, in_base, side='right'))
        hi = int(np.searchsorted(self._starts, in_base + in_count, side='left'))
        return self.channel.render(in_base, in_count, self._packed[lo:hi], self.sigma, self.mute_before, self.adc, copy=False)[0]


class ChannelizerSource:
    """Windows of channel ``k`` for ``DemodulatorRunner.run_device_stream``: iterates ``(device_ptr, nblocks)``.  Window w covers
    the channel's outputs ``w * B * stride .. w * B * stride + B * stride + overlap`` with ``stride = N - overlap`` and
    ``B = blocks_per_call``, and lies in the channeliser's output set ``w & 1`` (the loop's two-buffer contract: window w + 1 is
    written where window w - 1 was, after that batch has been collected).  ``wide`` is anything with ``render(in_base, in_count) ->
    device pointer`` of that span of the capture in the plan's sample format (``ChannelWide``).  Consecutive windows recompute
    the overlap they share -- an output is a function of its absolute position --, nothing is carried.  One source feeds one
    runner; every window is one channeliser call, which computes all K channels."""

    def __init__(self, channelizer, k, wide, N, overlap, blocks_per_call, nwindows):
        self.channelizer, self.k, self.wide = channelizer, int(k), wide
        self.N, self.overlap, self.B, self.nwindows = int(N), int(overlap), int(blocks_per_call), int(nwindows)
        self.stride = self.N - self.overlap
        self.count = self.B * self.stride + self.overlap
        if not 0 <= self.k < channelizer.K:
            raise ValueError(f'channel {k} of {channelizer.K}')
        if self.stride < 1 or self.B < 1 or self.nwindows < 0:
            raise ValueError('0 <= overlap < N, blocks_per_call >= 1, nwindows >= 0')
        # the longest input a window reads: one whose first output is far enough from 0 that nothing is clipped, in every phase
        # of its base modulo U (an integer plan has one: (count - 1) D + T)
        far = channelizer.T
        need = max(channelizer.needed_input(far + i, self.count)[1] for i in range(channelizer.interp))
        if self.count > channelizer.max_out or need > channelizer.max_in:
            raise ValueError(f'a window has {self.count} outputs: more than the channeliser was created for')

    def window_base(self, w):
        return w * self.B * self.stride

    def window_input(self, w):
        return self.channelizer.needed_input(self.window_base(w), self.count)

    def __len__(self):
        return self.nwindows

    def __iter__(self):
        if self.channelizer.backend != 'hip':
            raise ValueError("a ChannelizerSource yields device windows: the channeliser's back end is not 'hip'")
        for w in range(self.nwindows):
            in_base, in_count = self.window_input(w)
            ptr = self.wide.render(in_base, in_count)
            self.channelizer.process(in_base, (ptr, in_count), self.window_base(w), self.count, copy=False, buffer=w & 1)
            yield self.channelizer.device_output(w & 1, self.k)[0], self.B
