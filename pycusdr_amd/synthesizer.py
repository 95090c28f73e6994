"""The synthesiser behind the modulator: narrowband streams at a bank's ``baud * samplesPerSym`` rate are put onto the bins of a
raster of one wideband stream -- the dual of ``channelizer.UniformChannelizer``, with the arithmetic that one owns.  No reference
counterpart: the reference makes one narrowband stream per radio process (pyCuSDR.py:245-251).

A plan has ``M`` bins (8, 16, 32, 64, 128 or 256), an interpolation ``I`` with 2 <= I <= M (I need not divide M) and real float32
taps ``h[0..T)`` at the wide rate, 1 <= T <= 4096.  A call has a source array of complex64 and a list of placements
``(bin, start, src, length, gain)``: ``bin`` follows ``UniformChannelizer``'s convention (-M/2 <= bin < M, taken modulo M),
``start >= 0`` is an absolute position in the bin's narrow stream, ``gain`` a finite float32.  The stream of bin b is

    x_b[m] = fl(gain * source[src + m - start])       start <= m < start + length of a placement on bin b
    x_b[m] = 0                                        elsewhere

in float32, one rounding per component; a gain of 1 multiplies nothing.  Placements on one bin must not overlap in time (abutting
is allowed): an overlap is an error on both back ends.  With n the absolute wide position and ``(q, r) = divmod(n, I)``:

    w[n] = sum_b exp(+2 pi i b n / M) * sum_{j >= 0, r + jI < T} h[r + jI] x_b[q - j]
         = sum_{j >= 0, r + jI < T} h[r + jI] X_{q-j}[n mod M]
    X_m[s] = sum_b x_b[m] exp(+2 pi i b s / M)

zero-stuff by I, filter, then mix to the exact word ``(b << 64) // M``, without the zero products: one M-point transform per input
frame whatever the number of occupied bins, and ``ceil(T / I)`` real-by-complex multiply-adds per output, ``4 T + 5 M log2 M``
flops per frame.  ``w[n]`` is a pure function of (h, I, M, the placements, n): a span equals itself under any cut into calls, bit
for bit.

``backend='hip'`` is the mfb_synthesizer_* handle of include/mfbank.h (csrc/synthesize_uniform_kernels.hpp has the rules): each
output starts from (-0, -0) and adds j = 0, 1, ... in order, one fused multiply-add per component and tap, exactly the taps with
``r + jI < T``; a frame is transformed with the channeliser's ``chu_fft<M>`` on an image row that holds the placed samples in
natural bin order and zeros elsewhere.  ``backend='host'`` is the model rounded to complex64.  The model is the first sum in
float64, with gains as float32 values and exact phasors as ``Channelizer.model`` takes them; it returns ``(w complex128,
S float64)`` with ``S[n] = sum_j |h[r + jI]| * sum_b |x_b[q - j]|``, the scale of the device's error bound
``(ceil(T / I) + 3 log2 M + 3) * 2**-24 * S[n]`` per component.

``interp * design_taps(interp)`` is the prototype: unit pass-band gain, ``(T - 1) / 2`` wide samples of delay.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import OutputStage
from .modulator import phase
from .modulator.device import DeviceBatch         # noqa: F401  (a source ``set_source`` takes: callers name it from here)

_U = np.uint64
BINS, MAX_TAPS, MAX_FRAMES, MAX_OUT, MAX_SOURCE = (8, 16, 32, 64, 128, 256), 4096, 4096, 1 << 24, 1 << 26
LDS_BUDGET, MAX_TILE = 64 * 1024, 128

# mfb_synthesizer_placement as a numpy record
PLACEMENT_DTYPE = np.dtype([('start', '<i8'), ('src', '<i8'), ('length', '<i4'), ('bin', '<i4'), ('gain', '<f4'), ('reserved', '<i4')])
assert PLACEMENT_DTYPE.itemsize == C.sizeof(_lib.SynthesizerPlacement) == 32


def lds_bytes(M, I, T, F):
    """chsy_lds_bytes of csrc/channelize_plan.hpp: the image of F + ceil(T / I) - 1 frames, rows of M + 1 complex64; the twiddle
    table; the taps."""
    return ((F + -(-T // I) - 1) * (M + 1) + M) * 8 + 4 * T


def frames_per_workgroup(M, I, T):
    """chsy_frames of csrc/channelize_plan.hpp, restated: the largest F <= 128 whose image fits 64 KiB of LDS; 0 where not even
    F = 1 does, and the plan is refused.  Every plan with ceil(T / I) <= 17 fits."""
    F = MAX_TILE
    while F > 0 and lds_bytes(M, I, T, F) > LDS_BUDGET:
        F -= 1
    return F


def check_plan_synthesis(nbins, interp, taps):
    """The checks of mfb_synthesizer_create and mfb_synthesizer_set_plan, as ValueError: (M, I, taps float32)."""
    M, I = int(nbins), int(interp)
    if M not in BINS:
        raise ValueError(f'nbins is one of {BINS}')
    if not 2 <= I <= M:
        raise ValueError('2 <= interp <= nbins')
    taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if not 1 <= len(taps) <= MAX_TAPS or not np.all(np.isfinite(taps)):
        raise ValueError(f'1 .. {MAX_TAPS} finite taps')
    if not frames_per_workgroup(M, I, len(taps)):
        raise ValueError(f'ceil(T / I) = {-(-len(taps) // I)} frames of {M} bins do not fit a workgroup: fewer taps, or a larger interp')
    return M, I, taps


class Placement:
    """``length`` source samples from ``src`` on, times ``gain``, stand at the positions ``start ..`` of bin ``bin``'s stream."""
    __slots__ = ('bin', 'start', 'src', 'length', 'gain')

    def __init__(self, bin, start, src, length, gain=1.0):
        self.bin, self.start, self.src, self.length, self.gain = int(bin), int(start), int(src), int(length), float(np.float32(gain))

    def __repr__(self):
        return f'Placement(bin={self.bin}, start={self.start}, src={self.src}, length={self.length}, gain={self.gain})'


def check_placements(placements, nbins, source_len):
    """The checks of mfb_synthesizer_begin, as ValueError; ``bin`` already in [0, M)."""
    by_bin = {}
    for p in placements:
        if not 0 <= p.bin < nbins:
            raise ValueError(f'{p}: 0 <= bin < {nbins}')
        if not 1 <= p.length < 1 << 31:
            raise ValueError(f'{p}: 1 <= length < 2**31')
        if not 0 <= p.start < 1 << 62:
            raise ValueError(f'{p}: 0 <= start < 2**62')
        if not np.isfinite(p.gain):
            raise ValueError(f'{p}: gain is not finite')
        if p.src < 0 or p.src + p.length > source_len:
            raise ValueError(f'{p}: reads outside the source of {source_len} samples')
        by_bin.setdefault(p.bin, []).append(p)
    for ps in by_bin.values():
        ps.sort(key=lambda p: p.start)
        for a, b in zip(ps, ps[1:]):
            if b.start < a.start + a.length:
                raise ValueError(f'{a} and {b} overlap on bin {a.bin}')
    return by_bin


def pack_placements(placements):
    a = np.zeros(len(placements), dtype=PLACEMENT_DTYPE)
    for name in ('start', 'src', 'length', 'bin', 'gain'):
        a[name] = [getattr(p, name) for p in placements]
    return a


class UniformSynthesizer(OutputStage):
    """Streams onto a raster: bin b of ``nbins = M`` sits at ``b * fs / M`` of the wide stream of rate ``fs``; a narrow stream runs
    at ``fs / interp``.  The module docstring has the definition."""
    PREFIX = 'mfb_synthesizer'

    def __init__(self, fs, nbins, interp, taps, backend='hip', device=0, max_out=1 << 20, max_source=1 << 20, max_frames=4096):
        if backend not in ('hip', 'host'):
            raise ValueError("backend is 'hip' or 'host'")
        self.fs, self.backend, self.device = float(fs), backend, device
        self.nbins, self.interp, self.taps = check_plan_synthesis(nbins, interp, taps)
        self.T = len(self.taps)
        self.J = -(-self.T // self.interp)                    # taps of the longest branch: the frames an output reads
        self.max_out, self.max_source, self.max_frames = int(max_out), int(max_source), int(max_frames)
        if not (1 <= self.max_out <= MAX_OUT and 1 <= self.max_source <= MAX_SOURCE and 1 <= self.max_frames <= MAX_FRAMES):
            raise ValueError('max_out <= 2**24, max_source <= 2**26, max_frames <= 4096')
        self.source_len = 0
        self._src = self._keep = self._host = None
        self._buffer, self._count = 1, 0
        self.h = C.c_void_p()
        if backend == 'hip':
            self.lib = _lib.load()
            _lib.check(self.lib.mfb_synthesizer_create(C.byref(self.h), device, self.nbins, self.T, self.max_out, self.max_source,
                                                       self.max_frames), 'mfb_synthesizer_create')
            self._call('mfb_synthesizer_set_plan', self.interp, self.taps.ctypes.data, self.T)

    def close(self):
        super().close()
        self._keep = None

    @property
    def freqs_hz(self):
        """The centres of the M bins in index order, the upper half of the raster as negative frequencies: ``b * fs / M`` for
        b < M / 2, as ``UniformChannelizer.freqs_hz`` gives them for ``bins=None``."""
        b = np.arange(self.nbins, dtype=np.int64)
        return np.where(b >= self.nbins // 2, b - self.nbins, b) * (self.fs / self.nbins)

    def info(self):
        """(frames per workgroup F, the F + ceil(T / I) - 1 frames it transforms) of the plan in force (hip)."""
        a, b = C.c_int(), C.c_int()
        self._call('mfb_synthesizer_info', C.byref(a), C.byref(b))
        return a.value, b.value

    def elapsed_ms(self):
        ms = C.c_float()
        self._call('mfb_synthesizer_elapsed_ms', C.byref(ms))
        return ms.value

    def set_source(self, samples):
        """What the placements read: complex samples (copied in), a ``DeviceBatch`` of the device modulator, or ``(device_ptr,
        count)`` of complex64 -- both used in place, hip back end only, valid as long as their owner keeps them."""
        src = self._set_source(samples)
        if src is not None:                                   # (on either back end: ``model`` reads them)
            self._src = src.copy()

    def placement(self, bin, start, src, length, gain=1.0):
        """A descriptor; ``bin``: -M/2 <= bin < M, taken modulo M."""
        b = int(bin)
        if not -(self.nbins // 2) <= b < self.nbins:
            raise ValueError('-nbins / 2 <= bin < nbins')
        return Placement(b % self.nbins, start, src, length, gain)

    def needed_frames(self, out_base, out_count):
        """(first, count): the narrow positions that outputs out_base .. out_base + out_count read, clipped at 0: from
        ``out_base div I - (ceil(T / I) - 1)`` to ``(out_base + out_count - 1) div I``."""
        out_base, out_count = int(out_base), int(out_count)
        if out_base < 0 or out_count < 1:
            raise ValueError('out_base >= 0, out_count >= 1')
        first = max(0, out_base // self.interp - (self.J - 1))
        return first, (out_base + out_count - 1) // self.interp - first + 1

    def _checked(self, out_base, out_count, placements):
        out_base, out_count, placements = int(out_base), int(out_count), list(placements)
        if not 0 <= out_base < 1 << 62 or not 1 <= out_count <= self.max_out:
            raise ValueError(f'0 <= out_base < 2**62, 1 <= out_count <= max_out = {self.max_out}')
        if len(placements) > self.max_frames:
            raise ValueError(f'at most max_frames = {self.max_frames} placements')
        if not self.source_len:
            raise ValueError('no source set')
        return out_base, out_count, placements, check_placements(placements, self.nbins, self.source_len)

    def process(self, out_base, out_count, placements, copy=True, buffer=None):
        """The wide outputs out_base .. out_base + out_count.  ``copy``: complex64 [out_count]; not ``copy`` (hip): they stay in
        the handle's output set ``buffer`` (default: the one not written last), ask ``device_output`` for them."""
        self.begin(out_base, out_count, placements, buffer)
        return self.end(copy)

    def begin(self, out_base, out_count, placements, buffer=None):
        out_base, out_count, placements, by_bin = self._checked(out_base, out_count, placements)
        if self.backend == 'host':
            if self._src is None:
                raise ValueError("the 'host' back end reads host samples")
            self._host = self._model(out_base, out_count, by_bin)[0].astype(np.complex64)
            return
        self._buffer = (self._buffer ^ 1) if buffer is None else int(buffer)
        P = _lib.SynthesizerParams(out_base=out_base, out_count=out_count, buffer=self._buffer)
        pl = pack_placements(placements)
        self._call('mfb_synthesizer_begin', C.byref(P), pl.ctypes.data if len(pl) else None, len(pl))
        self._count = out_count

    def end(self, copy=True):
        return self._end(copy)                                # (not ``copy``: None; ask ``device_output``)

    def device_output(self, buffer):
        """(device_ptr, count) of output set ``buffer``."""
        return self._device_output(buffer)

    def model(self, out_base, out_count, placements, form='direct'):
        """The definition in float64 before rounding, from the host samples of ``set_source``: (w complex128 [out_count], S float64
        [out_count]).  ``form='direct'``: the first sum of the module docstring, stream by stream, filter then mix;
        ``'frames'``: the second, one M-point transform per input frame, then the filter."""
        if self._src is None:
            raise ValueError('the model reads host samples: set_source an array')
        if form not in ('direct', 'frames'):
            raise ValueError("form is 'direct' or 'frames'")
        out_base, out_count, _, by_bin = self._checked(out_base, out_count, placements)
        return self._model(out_base, out_count, by_bin, form)

    def streams(self, first, count, by_bin):
        """(bins, x complex128 [len(bins), count]): the streams of the occupied bins at the positions first .. first + count
        (first may be negative: zeros), gains applied in float32."""
        bins = sorted(by_bin)
        x = np.zeros((len(bins), count), dtype=np.complex128)
        for i, b in enumerate(bins):
            for p in by_bin[b]:
                lo, hi = max(p.start, first), min(p.start + p.length, first + count)
                if lo >= hi:
                    continue
                s = self._src[p.src + lo - p.start:p.src + hi - p.start]
                if p.gain != 1.0:
                    g = np.float32(p.gain)
                    s = (s.real * g) + 1j * (s.imag * g)         # float32 products, one rounding per component
                x[i, lo - first:hi - first] = s
        return bins, x

    def _model(self, out_base, out_count, by_bin, form='direct'):
        M, I, T, J = self.nbins, self.interp, self.T, self.J
        n = out_base + np.arange(out_count, dtype=np.int64)
        q, r = n // I, n % I
        first = int(q[0]) - (J - 1)                          # may be negative: those positions hold zeros
        bins, x = self.streams(first, int(q[-1]) - first + 1, by_bin)
        h = np.r_[self.taps.astype(np.float64), np.zeros(I)]     # (a branch's taps beyond T count as absent: they add exact zeros)
        at = q - first
        mag = np.abs(x).sum(axis=0)
        S = np.zeros(out_count, dtype=np.float64)
        for j in range(J):
            S += np.abs(h[np.minimum(r + j * I, T)]) * mag[at - j]
        w = np.zeros(out_count, dtype=np.complex128)
        step = _U((1 << 64) // M)
        if form == 'direct':
            for i, b in enumerate(bins):
                y = np.zeros(out_count, dtype=np.complex128)
                for j in range(J):
                    y += h[np.minimum(r + j * I, T)] * x[i, at - j]
                word = ((n % M) * b % M).astype(np.uint64) * step            # b n / M turns, exact
                w += np.where(word == 0, y, y * phase.words_to_iq(word))
            return w, S
        s = np.arange(M, dtype=np.int64)
        X = np.zeros((x.shape[1], M), dtype=np.complex128)       # X_m[s]
        for i, b in enumerate(bins):
            word = (s * b % M).astype(np.uint64) * step
            X += x[i][:, None] * np.where(word == 0, 1.0, phase.words_to_iq(word))[None, :]
        col = n % M
        for j in range(J):
            w += h[np.minimum(r + j * I, T)] * X[at - j, col]
        return w, S


class SynthesizerWide:
    """A ``UniformSynthesizer`` as the wideband capture of a ``channelizer.ChannelizerSource``: ``render(in_base, in_count)``
    renders that span of the wide stream on the device and returns its device pointer.  With a ``channel.Channel`` the span then
    passes through it as that channel's device source, as one frame at ``start = in_base`` with unit gain and no carrier, for its
    noise of standard deviation ``sigma`` per component and its ``adc`` grid."""

    def __init__(self, synth, placements, channel=None, sigma=0.0, adc=None):
        if synth.backend != 'hip' or (channel is not None and channel.backend != 'hip'):
            raise ValueError("the wideband capture is rendered with the 'hip' back end")
        self.synth, self.channel, self.sigma, self.adc = synth, channel, sigma, adc
        self.placements = list(placements)
        check_placements(self.placements, synth.nbins, synth.source_len)
        self._starts = np.array([p.start for p in self.placements], dtype=np.int64)
        self._ends = np.array([p.start + p.length for p in self.placements], dtype=np.int64)

    def render(self, in_base, in_count):
        first, count = self.synth.needed_frames(in_base, in_count)
        live = np.flatnonzero((self._ends > first) & (self._starts < first + count))
        self.synth.process(in_base, in_count, [self.placements[i] for i in live], copy=False)
        ptr, n = self.synth.device_output(self.synth._buffer)
        if self.channel is None:
            return ptr
        self.channel.set_source((ptr, n))
        frame = self.channel.frame(in_base, 0, n)
        return self.channel.render(in_base, n, [frame], self.sigma, 0, self.adc, copy=False)[0]
