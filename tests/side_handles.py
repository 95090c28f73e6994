"""The six side handles of libmfbank at the smallest shapes each accepts, through the C ABI directly: what
tests/test_gpu_handle_lifecycle.py walks and what test_gpu_configs.py fails the allocations of.

    sync finder            one 16-tap template, 64 bits
    combiner               max_bits 64, no slave
    modulator              an FSK table with sps 2, one frame of 2 bits
    channel                3 samples at an odd base, no frames
    channeliser            one channel, 3 taps, decimation 2
    uniform channeliser    8 bins, one selected
    synthesiser            8 bins, interpolation 2, 3 taps, 5 outputs, one placement
"""
import ctypes as C

import numpy as np

from pycusdr_amd import _lib

BINS, TAPS = 8, np.array([0.25, 0.5, 0.25], dtype=np.float32)
# name -> (create(lib, byref(out)) at device 0, the destroy function, the device allocations of the create)
CREATES = {
    'syncfinder': (lambda lib, out: lib.mfb_syncfinder_create(out, 0, SF_TMPL.ctypes.data, SF_T.ctypes.data, SF_THR.ctypes.data, 1, 64, 4),
                   'mfb_syncfinder_destroy', 3),                     # templates, results, bits
    'combiner': (lambda lib, out: lib.mfb_combiner_create(out, 0, 64, 0), 'mfb_combiner_destroy', 7),
    'modulator': (lambda lib, out: lib.mfb_modulator_create(out, 0, 2, 4), 'mfb_modulator_destroy', 6),
    'channel': (lambda lib, out: lib.mfb_channel_create(out, 0, 3, 4, 1), 'mfb_channel_destroy', 4),
    'channelizer': (lambda lib, out: lib.mfb_channelizer_create(out, 0, 1, 3, 16, 8), 'mfb_channelizer_destroy', 5),
    'channelizer_uniform': (lambda lib, out: lib.mfb_channelizer_create_uniform(out, 0, BINS, 1, 3, 64, 8), 'mfb_channelizer_destroy', 4),
    'synthesizer': (lambda lib, out: lib.mfb_synthesizer_create(out, 0, BINS, 3, 5, 4, 1), 'mfb_synthesizer_destroy', 6),
}

SF_TMPL = np.ones(16, dtype=np.int8)             # score[i] = sum_t tmpl[t] * bits[i - t]
SF_T, SF_THR = np.array([16], dtype=np.int32), np.array([16], dtype=np.int32)
SF_BITS = np.zeros(64, dtype=np.uint8)
SF_BITS[20:36] = 1                              # one position reaches 16: i = 35
SOURCE = (np.arange(1, 5) * (1 + 0.5j)).astype(np.complex64)
CHZ_IN = (np.arange(64) % 7 - 3 + 1j * (np.arange(64) % 5 - 2)).astype(np.complex64)


def create(lib, name):
    """A handle of CREATES[name]: the c_void_p."""
    h = C.c_void_p()
    _lib.check(CREATES[name][0](lib, C.byref(h)), name)
    return h


def destroy(lib, name, h):
    _lib.check(getattr(lib, CREATES[name][1])(h), CREATES[name][1])
