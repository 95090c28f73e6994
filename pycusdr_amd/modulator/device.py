"""ctypes wrapper of the mfb_modulator_* handle of include/mfbank.h (csrc/mod_kernels.hpp)."""
import ctypes as C

import numpy as np

from .. import _lib
from .._handle import Handle

MAX_FRAME_BITS, MAX_FRAMES, MAX_BITS, MAX_SAMPLES = 1 << 17, 4096, 1 << 22, 1 << 24


class DeviceBatch:
    """One batch left on the device: ``ptr`` complex64 [total], frame f at ``sample_off[f] .. sample_off[f + 1]``.
    ``frame_ptr(f)`` is what ``mfb_upload_device`` takes.  Valid until the modulator's next call."""

    def __init__(self, ptr, sample_off):
        self.ptr = ptr
        self.sample_off = sample_off
        self.total = int(sample_off[-1])

    def frame_ptr(self, f, offset=0):
        return self.ptr + 8 * (int(self.sample_off[f]) + offset)

    def frame_len(self, f):
        return int(self.sample_off[f + 1] - self.sample_off[f])


class DeviceModulator(Handle):
    PREFIX = 'mfb_modulator'

    def __init__(self, max_bits, max_samples, device=0):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.max_bits, self.max_samples = int(max_bits), int(max_samples)
        _lib.check(self.lib.mfb_modulator_create(C.byref(self.h), device, self.max_bits, self.max_samples), 'mfb_modulator_create')
        self._B = 0

    def set_lut(self, kind, lut_rad):
        lut = np.ascontiguousarray(lut_rad, dtype=np.float64)
        self._call('mfb_modulator_set_lut', kind, lut.ctypes.data, lut.shape[0], lut.shape[1])

    def set_pad(self, noise, pad_len, min_len):
        if noise is None:
            self._call('mfb_modulator_set_pad', None, 0, pad_len, min_len)
            return
        noise = np.ascontiguousarray(noise, dtype=np.complex64)
        self._call('mfb_modulator_set_pad', noise.ctypes.data, len(noise), pad_len, min_len)

    @staticmethod
    def pack(frames):
        """(bits uint8, bit_off int32 [B + 1]) of a list of 0/1 arrays: the form mfb_modulator_begin takes."""
        off = np.zeros(len(frames) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(f) for f in frames])
        bits = np.concatenate([np.asarray(f).reshape(-1) for f in frames]) if frames else np.zeros(0)
        return np.ascontiguousarray(bits != 0, dtype=np.uint8), off

    def begin(self, frames, dphi_rad=None):
        """frames: a list of 0/1 arrays; dphi_rad: one increment (rad per sample) per frame, or None."""
        self.begin_packed(*self.pack(frames), dphi_rad)

    def begin_packed(self, bits, off, dphi_rad=None):
        B = len(off) - 1
        d = None if dphi_rad is None else np.ascontiguousarray(dphi_rad, dtype=np.float64)
        if d is not None and len(d) != B:
            raise ValueError('one phase increment per frame')
        self._call('mfb_modulator_begin', bits.ctypes.data if len(bits) else None, off.ctypes.data, None if d is None else d.ctypes.data, B)
        self._B = B

    def end(self, copy=True, pinned=False):
        """Waits.  copy: (samples complex64 [total], sample_off); not copy: a DeviceBatch.  pinned: the samples are a view
        of the handle's page-locked buffer (valid until the next call) instead of a fresh array."""
        off = np.zeros(self._B + 1, dtype=np.int64)
        if not copy:
            self._call('mfb_modulator_end', None, off.ctypes.data)
            ptr, n = C.c_void_p(), C.c_int64()
            self._call('mfb_modulator_device_output', C.byref(ptr), C.byref(n))
            return DeviceBatch(ptr.value, off)
        host = C.POINTER(C.c_float)()
        self._call('mfb_modulator_host_buffer', C.byref(host))
        self._call('mfb_modulator_end', host, off.ctypes.data)
        view = np.ctypeslib.as_array(host, shape=(2 * self.max_samples,))[:2 * int(off[-1])].view(np.complex64)
        return (view if pinned else view.copy()), off

    def phase_words(self):
        """The test seam mfb_debug_mod_phase: the uint64 phase word of every sample of the batch ended last."""
        ptr, n = C.c_void_p(), C.c_int64()
        self._call('mfb_modulator_device_output', C.byref(ptr), C.byref(n))
        words = np.zeros(n.value, dtype=np.uint64)
        self._call('mfb_debug_mod_phase', words.ctypes.data, n.value)
        return words
