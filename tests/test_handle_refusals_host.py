"""What the six side handles of libmfbank (sync finder, combiner, modulator, channel, channeliser, synthesiser) refuse before they
touch a device, through the C ABI directly: the status code only.  A NULL handle, a NULL ``out``, a size of zero or below and a size
above a hard limit are each answered before the device check of a create, so these run on a machine without a GPU; what a valid
create returns there is not asserted.  The limits are read from the sources that define them."""
import ctypes as C
import glob
import os
import re

import pytest

from pycusdr_amd import _lib
from pycusdr_amd._lib import MFB_ERR_ARG, MFB_ERR_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _limits():
    """Every ``#define NAME <integer expression>`` of the library's sources and its C header."""
    out = {}
    files = glob.glob(os.path.join(ROOT, 'pycusdr_amd', 'csrc', '*.h*')) + [os.path.join(ROOT, 'include', 'mfbank.h')]
    for path in files:
        for name, expr in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\(?\d[\d \t<()]*?)[ \t]*(?://.*)?$', open(path).read(), re.M):
            out[name] = int(eval(expr, {'__builtins__': {}}))          # digits, <<, parentheses only
    return out


LIM = _limits()
SYNC_MAX_TAPS, SYNC_MAX_TEMPLATES = 4096, 16            # written out in mfb_syncfinder_create (mfbank.h states them)
BINS = 8


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_limits_are_read_from_the_sources():
    for name in ('CMB_MAX_BITS', 'MFB_COMBINE_MAX_SLAVES', 'MOD_MAX_BITS', 'MOD_MAX_SAMPLES', 'CHAN_MAX_SAMPLES', 'CHAN_MAX_SOURCE',
                 'CHAN_MAX_FRAMES', 'CHZ_MAX_CHANNELS', 'CHZ_MAX_TAPS', 'CHZ_MAX_IN', 'CHZ_MAX_OUT', 'CHU_MAX_TAPS', 'CHU_MAX_SET',
                 'CHSY_MAX_OUT', 'CHSY_MAX_SOURCE', 'CHSY_MAX_FRAMES'):
        assert LIM[name] >= 1, name


def _sf_create(lib, out, ntmpl=1, taps=16, max_bits=64, max_hits=4, tmpls=True):
    n = max(ntmpl, 1)
    T = (C.c_int * n)(*([taps] * n))
    thr = (C.c_int * n)(*([12] * n))
    big = (C.c_int8 * (max(taps, 1) * n))()
    return lib.mfb_syncfinder_create(out, 0, C.addressof(big) if tmpls else None, C.addressof(T), C.addressof(thr), ntmpl, max_bits, max_hits)


# (name, create(lib, out, *sizes), the valid sizes, [(index, limit)]: sizes[index] = limit + 1 is MFB_ERR_UNSUPPORTED)
def _creates():
    L = LIM
    return [
        ('combiner', lambda lib, out, *a: lib.mfb_combiner_create(out, 0, *a), (64, 0),
         [(0, L['CMB_MAX_BITS']), (1, L['MFB_COMBINE_MAX_SLAVES'])], {1: -1}),
        ('modulator', lambda lib, out, *a: lib.mfb_modulator_create(out, 0, *a), (64, 64),
         [(0, L['MOD_MAX_BITS']), (1, L['MOD_MAX_SAMPLES'])], {}),
        ('channel', lambda lib, out, *a: lib.mfb_channel_create(out, 0, *a), (3, 4, 1),
         [(0, L['CHAN_MAX_SAMPLES']), (1, L['CHAN_MAX_SOURCE']), (2, L['CHAN_MAX_FRAMES'])], {}),
        ('channelizer', lambda lib, out, *a: lib.mfb_channelizer_create(out, 0, *a), (1, 3, 16, 8),
         [(0, L['CHZ_MAX_CHANNELS']), (1, L['CHZ_MAX_TAPS']), (2, L['CHZ_MAX_IN']), (3, L['CHZ_MAX_OUT'])], {}),
        ('channelizer_uniform', lambda lib, out, *a: lib.mfb_channelizer_create_uniform(out, 0, *a), (BINS, 1, 3, 64, 8),
         [(1, BINS), (2, L['CHU_MAX_TAPS']), (3, L['CHZ_MAX_IN']), (4, L['CHZ_MAX_OUT'])], {}),
        ('synthesizer', lambda lib, out, *a: lib.mfb_synthesizer_create(out, 0, *a), (BINS, 3, 5, 4, 1),
         [(1, L['CHU_MAX_TAPS']), (2, L['CHSY_MAX_OUT']), (3, L['CHSY_MAX_SOURCE']), (4, L['CHSY_MAX_FRAMES'])], {}),
    ]


CREATES = _creates()
IDS = [c[0] for c in CREATES]


def _refused(create, lib, sizes, want):
    out = C.c_void_p(0xDEAD)                                         # a refused create clears it
    assert create(lib, C.byref(out), *sizes) == want, sizes
    assert out.value is None, sizes


@pytest.mark.parametrize('name,create,sizes,limits,floors', CREATES, ids=IDS)
def test_create_refuses_without_a_device(lib, name, create, sizes, limits, floors):
    assert create(lib, None, *sizes) == MFB_ERR_ARG                 # out = NULL
    for i in range(len(sizes)):
        for bad in ((floors[i],) if i in floors else (0, -1)):      # (a combiner takes 0 slaves)
            _refused(create, lib, sizes[:i] + (bad,) + sizes[i + 1:], MFB_ERR_ARG)
    for i, limit in limits:
        _refused(create, lib, sizes[:i] + (limit + 1,) + sizes[i + 1:], MFB_ERR_UNSUPPORTED)
        if i > 0:                                                   # a size below 1 is answered before a size above a limit
            _refused(create, lib, (0,) + sizes[1:i] + (limit + 1,) + sizes[i + 1:], MFB_ERR_ARG)


def test_create_refuses_other_bin_counts(lib):
    for bins in (1, 4, 12, 24, 512):
        _refused(CREATES[4][1], lib, (bins, 1, 3, 64, 8), MFB_ERR_UNSUPPORTED)
        _refused(CREATES[5][1], lib, (bins, 3, 5, 4, 1), MFB_ERR_UNSUPPORTED)
    # selected bins * outputs per channel above a set's capacity
    sel, per = 256, LIM['CHU_MAX_SET'] // 256 + 1
    assert per <= LIM['CHZ_MAX_OUT']
    _refused(CREATES[4][1], lib, (256, sel, 3, 64, per), MFB_ERR_UNSUPPORTED)


def test_syncfinder_create_refuses_without_a_device(lib):
    out = C.c_void_p(0xDEAD)
    assert _sf_create(lib, None) == MFB_ERR_ARG
    for kw in ({'ntmpl': 0}, {'ntmpl': -1}, {'ntmpl': SYNC_MAX_TEMPLATES + 1}, {'max_bits': 0}, {'max_bits': -1}, {'max_hits': 0},
               {'max_hits': -1}, {'taps': 0}, {'taps': -1}, {'taps': SYNC_MAX_TAPS + 1}, {'tmpls': False}):
        out.value = 0xDEAD
        assert _sf_create(lib, C.byref(out), **kw) == MFB_ERR_ARG, kw         # (this create has no MFB_ERR_UNSUPPORTED)
        assert out.value is None, kw


DESTROYS = ('mfb_syncfinder_destroy', 'mfb_combiner_destroy', 'mfb_modulator_destroy', 'mfb_channel_destroy', 'mfb_channelizer_destroy',
            'mfb_synthesizer_destroy')


@pytest.mark.parametrize('name', DESTROYS)
def test_destroy_null_is_an_argument_error(lib, name):
    assert getattr(lib, name)(None) == MFB_ERR_ARG


def _null_calls():
    """(name, arguments after the NULL handle): valid ones, so that the handle is what is refused."""
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    vp, i64, cint, cf, sz = C.c_void_p(), C.c_int64(), C.c_int(), C.c_float(), C.c_size_t()
    cp = _lib.CombineParams(variance_multiplier=3.0, min_length=16, master_len=64, num_slaves=0)
    chp = _lib.ChannelParams(base=1, count=3, buffer=0)
    zp = _lib.ChannelizerParams(in_base=0, out_base=0, in_count=16, out_count=4, input=2, device_input=p, buffer=0)
    sp = _lib.SynthesizerParams(out_base=0, out_count=5, buffer=0)
    fp = C.cast(p, C.POINTER(C.c_float))
    return [
        ('mfb_syncfinder_begin', (p, 64)), ('mfb_syncfinder_end', (p, p, p)),
        ('mfb_combiner_set_vote', (2, p, p, 64)), ('mfb_combiner_begin', (C.byref(cp), p, p, None, None)),
        ('mfb_combiner_end', (C.cast(p, C.POINTER(_lib.CombineResult)), p, p)),
        ('mfb_modulator_set_lut', (0, p, 2, 2)), ('mfb_modulator_set_pad', (None, 0, 0, 0)), ('mfb_modulator_begin', (p, p, None, 1)),
        ('mfb_modulator_end', (None, None)), ('mfb_modulator_device_output', (C.byref(vp), C.byref(i64))),
        ('mfb_modulator_host_buffer', (C.byref(C.POINTER(C.c_float)()),)), ('mfb_debug_mod_phase', (p, 4)),
        ('mfb_channel_set_source', (p, 4, 0)), ('mfb_channel_begin', (C.byref(chp), None, 0)), ('mfb_channel_end', (None,)),
        ('mfb_channel_device_output', (0, C.byref(vp), C.byref(i64))),
        ('mfb_channelizer_set_plan', (2, p, 3, p, 1, 0, 1.0)), ('mfb_channelizer_set_plan_rational', (1, 2, p, 3, p, 1, 0, 1.0)),
        ('mfb_channelizer_set_plan_uniform', (2, p, 3, p, 1, 0, 1.0)), ('mfb_channelizer_set_survey', (0, 0, 1.0)),
        ('mfb_channelizer_input_buffer', (0, C.byref(vp), C.byref(sz))), ('mfb_channelizer_begin', (C.byref(zp),)),
        ('mfb_channelizer_survey_begin', (C.byref(zp), 0)), ('mfb_channelizer_end', (None,)),
        ('mfb_channelizer_survey_end', (None, None, None, None)), ('mfb_channelizer_device_output', (0, 0, C.byref(vp), C.byref(i64))),
        ('mfb_channelizer_info', (C.byref(cint), C.byref(cint))),
        ('mfb_channelizer_survey_info', (C.byref(cint), C.byref(cint), C.byref(cint), C.byref(cf))),
        ('mfb_channelizer_elapsed_ms', (fp,)),
        ('mfb_synthesizer_set_plan', (2, p, 3)), ('mfb_synthesizer_set_source', (p, 4, 0)), ('mfb_synthesizer_begin', (C.byref(sp), None, 0)),
        ('mfb_synthesizer_end', (None,)), ('mfb_synthesizer_device_output', (0, C.byref(vp), C.byref(i64))),
        ('mfb_synthesizer_info', (C.byref(cint), C.byref(cint))), ('mfb_synthesizer_elapsed_ms', (fp,)),
    ], buf


def test_every_call_refuses_a_null_handle(lib):
    calls, keep = _null_calls()
    named = {n for n, _ in calls}
    # every entry point of the six handles that takes one, apart from create and destroy, is in the list
    for name in _lib.PROTOTYPES:
        if re.match(r'mfb_(syncfinder|combiner|modulator|channel|channelizer|synthesizer)_', name) and \
                not re.search(r'_create(_uniform)?$|_destroy$', name):
            assert name in named, name
    for name, args in calls:
        assert getattr(lib, name)(None, *args) == MFB_ERR_ARG, name
    del keep
