"""What the ctypes wrappers of libmfbank's stage handles share (csrc/stage_handle.hpp is the library's side of it): the handle and
its teardown, the status check of a call, and -- for the stages that have them -- the sample source and the two output sets."""
import ctypes as C

import numpy as np

from . import _lib


class Handle:
    """``h`` and ``lib`` of one ``<PREFIX>_*`` handle of include/mfbank.h.  ``h`` is NULL until the subclass has created it and after
    ``close``; a wrapper of the 'host' back end keeps it NULL and has no ``lib``."""
    PREFIX = None

    def _call(self, name, *args):
        _lib.check(getattr(self.lib, name)(self.h, *args), name)

    def close(self):
        if self.h:
            getattr(self.lib, self.PREFIX + '_destroy')(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OutputStage(Handle):
    """A stage that begins and ends calls on the 'hip' or the 'host' back end and leaves its outputs in one of two sets:
    ``_count`` outputs of the call begun last, ``_host`` the host back end's."""

    def _end(self, copy, *rows):
        """host: the model's outputs; ``copy``: complex64 [*rows, _count]; else None, the outputs stay on the device."""
        if self.backend == 'host':
            out, self._host = self._host, None
            return out
        out = np.empty(rows + (self._count,), dtype=np.complex64) if copy else None
        self._call(self.PREFIX + '_end', out.ctypes.data if copy else None)
        return out

    def _device_output(self, *which):
        ptr, n = C.c_void_p(), C.c_int64()
        self._call(self.PREFIX + '_device_output', *which, C.byref(ptr), C.byref(n))
        return ptr.value, n.value

    def _set_source(self, samples):
        """The body of ``set_source`` of the stages that read one (``max_source``, ``source_len``, ``_keep``): device memory -- a
        ``DeviceBatch`` or ``(device_ptr, count)`` -- is used in place and None returned; host samples are copied in (hip) and
        returned as complex64: whether to keep them is the caller's."""
        from .modulator.device import DeviceBatch
        name = self.PREFIX + '_set_source'
        if isinstance(samples, (DeviceBatch, tuple)):
            if self.backend != 'hip':
                raise ValueError("device memory is a source of the 'hip' back end")
            ptr, n = (samples.ptr, samples.total) if isinstance(samples, DeviceBatch) else (int(samples[0]), int(samples[1]))
            self._call(name, C.c_void_p(ptr), n, 1)
            self._keep, self.source_len = samples, n
            return None
        src = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
        if not 1 <= len(src) <= self.max_source:
            raise ValueError(f'1 <= source samples <= max_source = {self.max_source}')
        if self.backend == 'hip':
            self._call(name, src.ctypes.data, len(src), 0)
        self.source_len = len(src)
        return src
