"""The numpy model of the device peak clip (tests/clip_model.py) against the reference's fixture G9 and the host's
Demodulator._thresholdInput (reference DB:670-707), and the C ABI that carries the clip (include/mfbank.h)."""
import os
import re
import types

import numpy as np
import pytest

import clip_model as cm
from pycusdr_amd.demodulator.demodulator_base import Demodulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ('mfb_set_peak_clip', 'mfb_restart_peak_clip', 'mfb_get_block_clips', 'mfb_get_peak_clip_tail')
needs_fma = pytest.mark.skipif(not cm.fma3(), reason='numpy without FMA3 / AVX-512 computes |x| differently')


@needs_fma
def test_model_equals_g9():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_goldens.npz'))
    keys = sorted(k[:-4] for k in g.files if k.startswith('g9__') and k.endswith('__in'))
    assert len(keys) == 10
    for p in keys:
        x = g[p + '__in'].astype(np.complex64)
        idx = cm.clip(x, float(p.split('__s')[1]))
        assert np.array_equal(x.view(np.uint32), g[p + '__out'].view(np.uint32)), p
        assert np.array_equal(idx, g[p + '__clippedPeakIPure']), p


@needs_fma
@pytest.mark.parametrize('n', [4096, 1 << 15, 1 << 17, 1 << 20])
@pytest.mark.parametrize('scale', [4.5, 40.5, 4.3])
def test_model_equals_threshold_input(n, scale):
    rng = np.random.default_rng(n + int(scale * 10))
    x = cm.bursty(rng, n)
    y = x.copy()
    s = types.SimpleNamespace(peakThresholdScale=scale, Nfft=n)
    Demodulator._thresholdInput(s, y)
    z = x.copy()
    idx = cm.clip(z, scale)
    assert len(idx) > 0
    assert np.array_equal(y.view(np.uint32), z.view(np.uint32))
    assert np.array_equal(idx, s.clippedPeakIPure)


def test_gap_fill_is_shared():
    """clippedPeakI comes from one helper for the host clip and the device's indices."""
    from pycusdr_amd.demodulator.demodulator_base import fill_peak_gaps
    hot = np.array([3, 5, 50, 300, 301, 900])
    filled = fill_peak_gaps(hot, 1000, 100)
    assert list(filled) == [3, 4, 5] + list(range(5, 51))[1:] + [300, 301, 900]


def test_peak_clip_entry_points_declared_cited_exported():
    from pycusdr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mfbank.h')).read()
    import tu_source
    src = ''.join(tu_source.host_files().values())          # (the translation unit's host files: mfbank.hip and its parts)
    assert os.path.exists(os.path.join(ROOT, 'pycusdr_amd', 'csrc', 'clip_kernels.hpp'))
    for name in ENTRY:
        m = re.search(r'((?:/\*(?:(?!\*/).)*\*/\s*)+)int ' + name + r'\(', hdr, re.S)
        assert m, name
        assert 'DB:670-707' in m.group(1), name
        assert re.search(r'extern "C" int ' + name + r'\(', src), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in ENTRY:
        assert hasattr(lib, name), name
    assert 'on the host, block by block' not in hdr
