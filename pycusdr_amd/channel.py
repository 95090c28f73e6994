"""The radio channel between ``Modulator`` and the receive loop: frames placed at their arrival times in one continuous
stream, each on its own carrier with a linear frequency drift, white Gaussian noise underneath, optionally an ADC's grid.

The stream is a pure function of (seed, frames, source, parameters, absolute sample position): ``render(base, count, ...)``
gives the same samples whatever the spans it is asked for in, bit for bit.  Per absolute sample n

    out[n] = adc(gain_f * src[src_f + k] * exp(2 pi i phi_f(k) / 2**64) + sigma * (gI(n) + i gQ(n)))    k = n - start_f
    out[n] = adc(sigma * (gI(n) + i gQ(n)))                                                             outside every frame
    out[n] = 0                                                                                          n < mute_before

with phi_f(k) = phase0 + k * freq + (k (k - 1) / 2) * rate in uint64 turns modulo 2**64 (the convention of
``modulator/phase.py``), Philox4x32-10 noise keyed by the seed and counted by n >> 1, and Box-Muller on its words
(csrc/channel_kernels.hpp has the rules).  ``backend='hip'`` is the mfb_channel_* handle of include/mfbank.h;
``backend='host'`` is the model: the same integers (Philox words, the uniform, the phase words) with numpy, the floating-point
part in float64, rounded to complex64 at the end.  It restates ``signals.awgn`` (reference create_signals.py:115-141) and the
pad-and-mix of ``signals.get_padded_packet`` (create_signals.py:197-198).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import OutputStage
from .modulator import phase
from .modulator.device import DeviceBatch         # noqa: F401  (a source ``set_source`` takes: callers name it from here)

_U = np.uint64
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = _U(0xFFFFFFFF)
MAX_SAMPLES, MAX_SOURCE, MAX_FRAMES = 1 << 24, 1 << 26, 1 << 20
R_MAX = float(np.sqrt(48 * np.log(2.0)))          # the largest radius: u = 2**-24


def philox4x32(counter, key, rounds=10):
    """Philox4x32 of ``counter`` uint32 [..., 4] under ``key`` uint32 [..., 2] (broadcast): uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = _U(_M0) * c0, _U(_M1) * c2                  # 32 x 32 -> 64: no overflow
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> _U(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _U(_W0)) & _MASK, (k1 + _U(_W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise_words(seed, n):
    """The two words (uint32 [len(n), 2]) of absolute samples ``n``: words 2 (n & 1), 2 (n & 1) + 1 of block n >> 1."""
    n = np.asarray(n, dtype=np.uint64)
    p = n >> _U(1)
    ctr = np.stack([p & _MASK, p >> _U(32), np.zeros_like(p), np.zeros_like(p)], axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    odd = (n & _U(1)).astype(bool)
    return np.where(odd[:, None], w[:, 2:], w[:, :2])


def uniform_of(w0):
    """u = ((w >> 8) + 1) * 2**-24 in (0, 1]."""
    return ((np.asarray(w0, dtype=np.uint64) >> _U(8)) + _U(1)).astype(np.float64) * 2.0 ** -24


def radius_of(w0):
    return np.sqrt(-2.0 * np.log(uniform_of(w0)))


def normals_of(w0, w1):
    """(gI, gQ) float64 of word pairs: radius from the first word, angle 2 pi w1 / 2**32 from the second."""
    return radius_of(w0) * phase.words_to_iq(np.asarray(w1, dtype=np.uint64) << _U(32))


def signed_quantise(v):
    """rad -> uint64 turns; a negative value is the two's complement of its magnitude's word (so -v and v sum to 0 exactly and a
    small negative rate keeps its precision)."""
    v = np.asarray(v, dtype=np.float64)
    q = phase.quantise(np.abs(v))
    with np.errstate(over='ignore'):
        return np.where(v < 0, _U(0) - q, q).astype(np.uint64)


def phase_words(phase0, freq, rate, k):
    """phi(k) = phase0 + k freq + (k (k - 1) / 2) rate modulo 2**64, k uint64 < 2**31."""
    k = np.asarray(k, dtype=np.uint64)
    tri = np.where(k & _U(1), k * ((k - _U(1)) >> _U(1)), (k >> _U(1)) * (k - _U(1)))      # exact: < 2**61 (0 for k = 0)
    with np.errstate(over='ignore'):
        return _U(phase0) + k * _U(freq) + tri * _U(rate)


def adc_quantise(x, bits, scale):
    """rint(x / scale) to even, saturated to the signed range of ``bits``, times scale: float32 in, float32 out -- what the
    sc16 / sc8 input path computes from the integers."""
    hi = float((1 << (bits - 1)) - 1)
    q = np.clip(np.rint(np.asarray(x, dtype=np.float32) * np.float32(1.0 / scale)), -hi - 1, hi).astype(np.int32)
    return q.astype(np.float32) * np.float32(scale)


def _check_adc(adc):
    if adc is None:
        return 0, 1.0
    bits, scale = adc
    m, _ = np.frexp(np.float32(scale))
    if bits not in (8, 16) or not (np.isfinite(scale) and scale > 0 and m == 0.5):
        raise ValueError('adc = (8 or 16, a power of two)')
    return int(bits), float(scale)


class Frame:
    """One descriptor: ``length`` source samples from ``src`` arrive at absolute position ``start``."""
    __slots__ = ('start', 'src', 'length', 'gain', 'phase0', 'freq', 'rate')

    def __init__(self, start, src, length, gain, phase0, freq, rate):
        self.start, self.src, self.length, self.gain = int(start), int(src), int(length), float(gain)
        self.phase0, self.freq, self.rate = int(phase0), int(freq), int(rate)

    def __repr__(self):
        return f'Frame(start={self.start}, src={self.src}, length={self.length}, gain={self.gain})'


# mfb_channel_frame as a numpy record: a list of descriptors packed once goes to the library as it is
FRAME_DTYPE = np.dtype([('start', '<i8'), ('src', '<i8'), ('length', '<i4'), ('gain', '<f4'), ('phase0', '<u8'), ('freq', '<u8'), ('rate', '<u8')])
assert FRAME_DTYPE.itemsize == C.sizeof(_lib.ChannelFrame) == 48


def pack_frames(frames):
    """The descriptors as one array of FRAME_DTYPE: what ``render`` takes in place of the list when the same frames are rendered
    window after window (a slice of it is a window's frames; the library checks them, the Python loop over them is saved)."""
    a = np.zeros(len(frames), dtype=FRAME_DTYPE)
    for name in FRAME_DTYPE.names:
        a[name] = [getattr(f, name) for f in frames]
    return a


def unpack_frames(packed):
    return [Frame(*(r[name] for name in FRAME_DTYPE.names)) for r in packed]


def check_frames(frames, source_len):
    """The checks of mfb_channel_begin, as ValueError."""
    free_from = 0
    for f in frames:
        if f.length < 1 or f.length >= 1 << 31:
            raise ValueError(f'{f}: 1 <= length < 2**31')
        if f.start < 0:
            raise ValueError(f'{f}: start >= 0')
        if f.start < free_from:
            raise ValueError(f'{f}: frames are sorted by start and do not overlap')
        if not np.isfinite(f.gain):
            raise ValueError(f'{f}: gain is not finite')
        if f.src < 0 or f.src + f.length > source_len:
            raise ValueError(f'{f}: reads outside the source of {source_len} samples')
        free_from = f.start + f.length


class Channel(OutputStage):
    PREFIX = 'mfb_channel'

    def __init__(self, fs, seed=0, backend='hip', device=0, max_samples=1 << 20, max_source=1 << 20, max_frames=4096):
        if backend not in ('hip', 'host'):
            raise ValueError("backend is 'hip' or 'host'")
        self.fs, self.seed, self.backend, self.device = float(fs), int(seed) & 0xFFFFFFFFFFFFFFFF, backend, device
        self.max_samples, self.max_source, self.max_frames = int(max_samples), int(max_source), int(max_frames)
        if not (1 <= self.max_samples <= MAX_SAMPLES and 1 <= self.max_source <= MAX_SOURCE and 1 <= self.max_frames <= MAX_FRAMES):
            raise ValueError('max_samples <= 2**24, max_source <= 2**26, max_frames <= 2**20')
        self.source_len = 0
        self._src = self._keep = None
        self._buffer = 1
        self.h = C.c_void_p()
        if backend == 'hip':
            self.lib = _lib.load()
            _lib.check(self.lib.mfb_channel_create(C.byref(self.h), device, self.max_samples, self.max_source, self.max_frames),
                       'mfb_channel_create')

    def set_source(self, samples):
        """What the frames read: complex samples (copied in), or a ``DeviceBatch`` of the device modulator, used in place
        (hip back end only; it stays valid until that modulator's next call), or ``(device_ptr, count)`` of complex64, used in
        place likewise (a synthesiser's ``device_output``)."""
        src = self._set_source(samples)
        if src is not None and self.backend == 'host':        # (only the model reads the host's samples again)
            self._src = src.copy()

    def frame(self, start, src, length, gain=1.0, doppler_hz=0.0, rate_hz_per_s=0.0, phase_rad=0.0):
        """A descriptor: the carrier is at ``doppler_hz`` at the frame's first sample and moves by ``rate_hz_per_s``."""
        return Frame(start, src, length, gain, signed_quantise(phase_rad), signed_quantise(phase.TWO_PI * doppler_hz / self.fs),
                     signed_quantise(phase.TWO_PI * rate_hz_per_s / self.fs ** 2))

    @staticmethod
    def sigma_for(snr_db, power=1.0, measured=True):
        """The standard deviation per component that ``signals.awgn`` gives complex noise at ``snr_db``: ``power`` is the signal's
        mean |x|^2 (``measured``, create_signals.py:127-131), else the SNR is taken against unit power."""
        snr = float(snr_db)
        if measured:
            snr = snr - 10 * np.log10(power)
        return float(np.sqrt(10 ** (-snr / 10) / 2))

    def _checked(self, base, count, frames, sigma, mute_before):
        base, count, mute_before, sigma = int(base), int(count), int(mute_before), float(sigma)
        if not 1 <= count <= self.max_samples:
            raise ValueError(f'1 <= count <= max_samples = {self.max_samples}')
        if not 0 <= base < 1 << 62 or mute_before < 0:
            raise ValueError('0 <= base < 2**62, mute_before >= 0')
        if not (np.isfinite(sigma) and sigma >= 0):
            raise ValueError('sigma >= 0')
        packed = isinstance(frames, np.ndarray) and frames.dtype == FRAME_DTYPE
        if packed and self.backend == 'hip':
            if len(frames) > self.max_frames:
                raise ValueError(f'at most max_frames = {self.max_frames} frames')
            return base, count, np.ascontiguousarray(frames), sigma, mute_before      # (mfb_channel_begin checks them)
        frames = unpack_frames(frames) if packed else list(frames)
        if len(frames) > self.max_frames:
            raise ValueError(f'at most max_frames = {self.max_frames} frames')
        if frames and not self.source_len:
            raise ValueError('frames given, but no source set')
        check_frames(frames, self.source_len)
        return base, count, frames, sigma, mute_before

    def render(self, base, count, frames=(), sigma=0.0, mute_before=0, adc=None, copy=True, buffer=None):
        """Absolute samples base .. base + count; ``frames``: a list of descriptors, or ``pack_frames`` of one.  ``copy``:
        complex64 [count]; not ``copy`` (hip): ``(device_ptr, count)`` of
        the window, left in the handle's buffer ``buffer`` (default: the one not rendered last)."""
        self.begin(base, count, frames, sigma, mute_before, adc, buffer)
        return self.end(copy)

    def begin(self, base, count, frames=(), sigma=0.0, mute_before=0, adc=None, buffer=None):
        base, count, frames, sigma, mute_before = self._checked(base, count, frames, sigma, mute_before)
        bits, scale = _check_adc(adc)
        if self.backend == 'host':
            self._host = self._render_host(base, count, frames, sigma, mute_before, bits, scale)
            return
        self._buffer = (self._buffer ^ 1) if buffer is None else int(buffer)
        P = _lib.ChannelParams(base=base, mute_before=mute_before, seed=self.seed, count=count, buffer=self._buffer, sigma=sigma,
                               adc_scale=scale, adc_bits=bits)
        F = frames if isinstance(frames, np.ndarray) else pack_frames(frames)
        self._call('mfb_channel_begin', C.byref(P), F.ctypes.data if len(F) else None, len(F))
        self._count = count

    def end(self, copy=True):
        out = self._end(copy)
        return out if copy or self.backend == 'host' else self.device_output(self._buffer)     # (not ``copy``: where the window is)

    def device_output(self, buffer):
        return self._device_output(buffer)

    def model_parts(self, base, count, frames, sigma):
        """The float64 model before rounding, for error bounds: (signal complex128 [count], noise complex128 [count] =
        sigma * g, radius float64 [count])."""
        n = np.arange(base, base + count, dtype=np.uint64)
        sig = np.zeros(count, dtype=np.complex128)
        for f in frames:
            lo, hi = max(f.start, base), min(f.start + f.length, base + count)
            if lo >= hi:
                continue
            k = np.arange(lo - f.start, hi - f.start, dtype=np.uint64)
            s = self._src[f.src + int(k[0]):f.src + int(k[-1]) + 1].astype(np.complex128)
            w = phase_words(f.phase0, f.freq, f.rate, k)
            rot = np.where(w == 0, s, s * phase.words_to_iq(w))
            sig[lo - base:hi - base] = np.float64(np.float32(f.gain)) * rot
        if sigma == 0:
            return sig, np.zeros(count, dtype=np.complex128), np.zeros(count)
        w = noise_words(self.seed, n)
        return sig, np.float64(np.float32(sigma)) * normals_of(w[:, 0], w[:, 1]), radius_of(w[:, 0])

    def _render_host(self, base, count, frames, sigma, mute_before, bits, scale):
        sig, noise, _ = self.model_parts(base, count, frames, sigma)
        v = sig + noise if sigma else sig
        out = v.astype(np.complex64)
        if bits:
            out = (adc_quantise(out.real, bits, scale) + 1j * adc_quantise(out.imag, bits, scale)).astype(np.complex64)
        muted = np.arange(base, base + count) < mute_before if mute_before > base else None
        if muted is not None:
            out[muted] = 0
        return out


class LoopbackSource:
    """Windows of the stream for ``DemodulatorRunner.run_device_stream``: iterates ``(device_ptr, nblocks)``.  Window w spans the
    absolute samples ``w * B * stride .. w * B * stride + B * stride + overlap`` with ``stride = N - overlap`` and
    ``B = blocks_per_call``, and lies in the channel's buffer ``w & 1``: two consecutive windows each render the ``overlap``
    samples they share (the stream is a function of the absolute position), nothing is carried.  ``mute_before`` defaults to
    ``overlap``: the stream begins with the zeros the host loop starts from.  A window is rendered when the iterator is asked for
    it, into the buffer of window w - 2 -- whose batch the loop has collected by then (``run_device_stream``)."""

    def __init__(self, channel, frames, N, overlap, blocks_per_call, nwindows, sigma=0.0, mute_before=None, adc=None, keep_host=False):
        self.channel, self.frames = channel, list(frames)
        self.keep_host, self.host_windows = keep_host, []
        self.N, self.overlap, self.B, self.nwindows = int(N), int(overlap), int(blocks_per_call), int(nwindows)
        self.stride = self.N - self.overlap
        self.count = self.B * self.stride + self.overlap
        self.sigma, self.adc = sigma, adc
        self.mute_before = self.overlap if mute_before is None else int(mute_before)
        if channel.backend != 'hip':
            raise ValueError("a LoopbackSource renders with the 'hip' back end")
        if self.count > channel.max_samples:
            raise ValueError(f'a window has {self.count} samples; the channel was created for {channel.max_samples}')
        check_frames(self.frames, channel.source_len)
        self._starts = np.array([f.start for f in self.frames], dtype=np.int64)
        self._ends = np.array([f.start + f.length for f in self.frames], dtype=np.int64)
        self._packed = pack_frames(self.frames)

    def window_base(self, w):
        return w * self.B * self.stride

    def window_frames(self, w):
        """The frames that touch window w (the descriptors are sorted: one slice)."""
        base = self.window_base(w)
        lo = int(np.searchsorted(self._ends, base, side='right'))
        hi = int(np.searchsorted(self._starts, base + self.count, side='left'))
        return self._packed[lo:hi]

    def render(self, w, copy=False):
        return self.channel.render(self.window_base(w), self.count, self.window_frames(w), self.sigma, self.mute_before, self.adc,
                                   copy=copy, buffer=w & 1)

    def __len__(self):
        return self.nwindows

    def __iter__(self):
        for w in range(self.nwindows):
            if self.keep_host:
                self.host_windows.append(self.render(w, copy=True))
                ptr, _ = self.channel.device_output(w & 1)
            else:
                ptr, _ = self.render(w)
            yield ptr, self.B
