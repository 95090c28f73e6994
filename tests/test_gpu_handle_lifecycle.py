"""The begin / end state machine that the six side handles of libmfbank share, walked once per handle at the smallest shapes each
accepts (tests/side_handles.py), through the C ABI directly: the status codes only, and that a call repeated after ``end(NULL)``
gives the same bytes.  Where two refusals apply at once the order of the checks in the library decides, and the code asserted is
the one the library gave when these walks were written; profiles/stage_handles.md lists them."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd._lib import MFB_ERR_ARG, MFB_ERR_STATE, MFB_OK
from side_handles import BINS, CHZ_IN, SF_BITS, SOURCE, TAPS, create, destroy

pytestmark = pytest.mark.gpu
OK, ARG, STATE = MFB_OK, MFB_ERR_ARG, MFB_ERR_STATE


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


class Walk:
    """One handle for the length of a test; ``w.name(args...)`` is ``mfb_<prefix>_name(handle, args...)``: the status."""

    def __init__(self, lib, kind, prefix):
        self.lib, self.kind, self.prefix = lib, kind, prefix
        self.h = create(lib, kind)

    def __getattr__(self, name):
        fn = getattr(self.lib, f'mfb_{self.prefix}_{name}')
        return lambda *a: fn(self.h, *a)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        destroy(self.lib, self.kind, self.h)


def _dev_out(w, *sel):
    """device_output of set (and channel) ``sel``: the status."""
    ptr, n = C.c_void_p(), C.c_int64()
    return w.device_output(*sel, C.byref(ptr), C.byref(n))


def _elapsed(w):
    ms = C.c_float(-1.0)
    return w.elapsed_ms(C.byref(ms))


def test_syncfinder(lib):
    counts, idx, score = np.zeros(1, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    out = (counts.ctypes.data, idx.ctypes.data, score.ctypes.data)
    with Walk(lib, 'syncfinder', 'syncfinder') as w:
        assert w.end(*out) == STATE                                  # before any begin
        assert w.begin(SF_BITS.ctypes.data, 64) == OK
        assert w.begin(SF_BITS.ctypes.data, 64) == STATE             # busy
        assert w.begin(SF_BITS.ctypes.data, 0) == ARG                # the argument error comes first
        assert w.end(None, idx.ctypes.data, score.ctypes.data) == ARG        # ... and leaves the call in flight
        assert w.end(*out) == OK
        first = counts.tobytes() + idx.tobytes() + score.tobytes()
        assert counts[0] == 1 and idx[0] == 35 and score[0] == 16, (counts, idx, score)      # sixteen ones end at bit 35
        assert w.end(*out) == STATE
        assert w.begin(SF_BITS.ctypes.data, 64) == OK
        assert w.end(*out) == OK
        assert counts.tobytes() + idx.tobytes() + score.tobytes() == first


def test_combiner(lib):
    bits = (np.arange(64) % 3 == 0).astype(np.uint8)
    trust = np.full(64, 5, dtype=np.int8)
    lut_b, lut_t = np.zeros(64, np.uint8), np.zeros(64, np.int8)
    P = _lib.CombineParams(variance_multiplier=3.0, min_length=16, master_len=64, num_slaves=0)
    res, ob, ot = _lib.CombineResult(), np.zeros(64, np.uint8), np.zeros(64, np.int8)
    begin = (C.byref(P), bits.ctypes.data, trust.ctypes.data, None, None)
    end = (C.byref(res), ob.ctypes.data, ot.ctypes.data)
    with Walk(lib, 'combiner', 'combiner') as w:
        assert w.end(*end) == STATE
        assert w.set_vote(2, lut_b.ctypes.data, lut_t.ctypes.data, 64) == OK
        assert w.begin(*begin) == OK
        assert w.begin(*begin) == STATE
        assert w.set_vote(2, lut_b.ctypes.data, lut_t.ctypes.data, 64) == STATE
        assert w.set_vote(2, lut_b.ctypes.data, lut_t.ctypes.data, 63) == ARG        # the argument error comes first
        bad = _lib.CombineParams(variance_multiplier=3.0, min_length=16, master_len=65, num_slaves=0)
        assert w.begin(C.byref(bad), bits.ctypes.data, trust.ctypes.data, None, None) == ARG
        assert w.end(*end) == OK
        first = bytes(res) + ob.tobytes() + ot.tobytes()
        assert res.out_len == 64 and np.array_equal(ob, bits)       # no slave: the master's bits
        assert w.end(*end) == STATE
        assert w.begin(*begin) == OK
        assert w.end(*end) == OK
        assert bytes(res) + ob.tobytes() + ot.tobytes() == first


def test_modulator(lib):
    lut = np.array([[-0.3, -0.3], [0.3, 0.3]], dtype=np.float64)     # MFB_MOD_FSK: 2 rows, sps 2
    bits, off = np.array([1, 0], dtype=np.uint8), np.array([0, 2], dtype=np.int32)
    out, soff, words = np.zeros(4, np.complex64), np.zeros(2, np.int64), np.zeros(4, np.uint64)
    begin = (bits.ctypes.data, off.ctypes.data, None, 1)
    with Walk(lib, 'modulator', 'modulator') as w:
        phase = lambda: lib.mfb_debug_mod_phase(w.h, words.ctypes.data, 4)           # noqa: E731
        assert w.end(None, None) == STATE
        assert w.begin(*begin) == STATE                              # no table yet
        assert w.set_lut(0, lut.ctypes.data, 2, 2) == OK
        assert w.set_pad(None, 0, 0, 0) == OK
        assert _dev_out(w) == STATE and phase() == STATE             # before the first end
        assert w.begin(*begin) == OK
        assert w.begin(*begin) == STATE
        assert w.set_lut(0, lut.ctypes.data, 2, 2) == STATE
        assert w.set_pad(None, 0, 0, 0) == STATE
        assert w.set_lut(0, lut.ctypes.data, 3, 2) == ARG and w.set_pad(None, 0, -1, 0) == ARG       # argument errors come first
        assert w.begin(bits.ctypes.data, off.ctypes.data, None, 0) == ARG
        assert _dev_out(w) == STATE and phase() == STATE             # still before the first end
        assert w.end(out.ctypes.data, soff.ctypes.data) == OK
        first = out.tobytes() + soff.tobytes()
        assert list(soff) == [0, 4] and np.allclose(np.abs(out), 1.0, atol=1e-6)
        assert _dev_out(w) == OK and phase() == OK
        assert w.end(None, None) == STATE
        assert w.begin(*begin) == OK
        assert _dev_out(w) == STATE and phase() == STATE             # in flight
        assert w.end(None, None) == OK                               # clears busy
        assert _dev_out(w) == OK
        assert w.set_lut(0, lut.ctypes.data, 2, 2) == OK             # a new table: the finished batch belonged to the old one
        assert _dev_out(w) == STATE and phase() == STATE
        out[:] = 0
        assert w.begin(*begin) == OK
        assert w.end(out.ctypes.data, soff.ctypes.data) == OK
        assert out.tobytes() + soff.tobytes() == first


def test_channel(lib):
    out = np.zeros(3, np.complex64)
    P = [_lib.ChannelParams(base=1, mute_before=0, seed=5, count=3, buffer=b, sigma=1.0, adc_scale=1.0, adc_bits=0) for b in (0, 1)]
    frame = _lib.ChannelFrame(start=1, src=0, length=2, gain=1.0)
    with Walk(lib, 'channel', 'channel') as w:
        assert w.end(None) == STATE
        assert _dev_out(w, 0) == STATE and _dev_out(w, 1) == STATE   # never written
        assert w.begin(C.byref(P[0]), C.byref(frame), 1) == STATE    # frames, but no source
        assert w.begin(C.byref(P[0]), None, 0) == OK
        assert w.begin(C.byref(P[0]), None, 0) == STATE
        bad = _lib.ChannelParams(base=1, seed=5, count=0, buffer=0, sigma=1.0)
        assert w.begin(C.byref(bad), None, 0) == ARG                 # a bad count while busy: the argument error comes first
        assert w.set_source(SOURCE.ctypes.data, 4, 0) == STATE
        assert w.set_source(SOURCE.ctypes.data, 5, 0) == ARG         # above max_source: the argument error comes first
        assert _dev_out(w, 0) == STATE                               # in flight
        assert _dev_out(w, 1) == STATE                               # never written
        assert _dev_out(w, 2) == ARG
        assert w.end(out.ctypes.data) == OK
        first = out.tobytes()
        assert np.all(out != 0)                                      # noise everywhere
        assert w.end(None) == STATE
        assert _dev_out(w, 0) == OK
        assert w.set_source(SOURCE.ctypes.data, 4, 0) == OK
        assert w.begin(C.byref(P[1]), None, 0) == OK
        assert _dev_out(w, 0) == OK                                  # the other, finished set while a call is in flight
        assert _dev_out(w, 1) == STATE
        assert w.end(None) == OK                                     # clears busy
        assert _dev_out(w, 1) == OK
        out[:] = 0
        assert w.begin(C.byref(P[0]), None, 0) == OK
        assert w.end(out.ctypes.data) == OK
        assert out.tobytes() == first


def _pinned(w, which, samples):
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert w.input_buffer(which, C.byref(ptr), C.byref(nbytes)) == OK
    buf = np.frombuffer((C.c_uint8 * nbytes.value).from_address(ptr.value), dtype=np.complex64)
    buf[:len(samples)] = samples


def _channelizer_walk(w, set_plan, other_plans, in_count):
    """The part of the walk that a plain and a uniform handle share; set_plan(): the handle's own, with valid arguments;
    other_plans: [(call, status)] of the other kinds' set_plan on this handle, with and without a call in flight."""
    out = np.zeros(4, np.complex64)
    P = [_lib.ChannelizerParams(in_base=0, out_base=0, in_count=in_count, out_count=4, input=0, buffer=b) for b in (0, 1)]
    assert w.end(None) == STATE
    assert w.begin(C.byref(P[0])) == STATE                           # no plan
    assert _elapsed(w) == STATE
    assert set_plan() == OK
    for call, status in other_plans:
        assert call() == status
    assert w.begin(C.byref(P[0])) == STATE                           # the page-locked buffer was never asked for
    _pinned(w, 0, CHZ_IN[:in_count])
    assert _elapsed(w) == STATE                                      # before the first finished call
    assert w.begin(C.byref(P[0])) == OK
    assert w.begin(C.byref(P[0])) == STATE
    assert set_plan() == STATE
    for call, status in other_plans:
        assert call() == status
    bad = _lib.ChannelizerParams(in_base=0, out_base=0, in_count=0, out_count=4, input=0, buffer=0)
    assert w.begin(C.byref(bad)) == ARG                              # the argument error comes first
    assert _elapsed(w) == STATE                                      # busy
    assert _dev_out(w, 0, 0) == STATE                                # in flight
    assert _dev_out(w, 1, 0) == STATE                                # never written
    assert w.end(out.ctypes.data) == OK
    first = out.tobytes()
    assert np.any(out != 0)
    assert w.end(None) == STATE
    assert _elapsed(w) == OK
    assert _dev_out(w, 0, 0) == OK and _dev_out(w, 0, 1) == STATE    # (a channel the plan does not have)
    assert w.begin(C.byref(P[1])) == OK
    assert _dev_out(w, 0, 0) == OK                                   # the other, finished set while a call is in flight
    assert _dev_out(w, 1, 0) == STATE
    assert w.end(None) == OK                                         # clears busy
    assert _dev_out(w, 1, 0) == OK
    out[:] = 0
    assert w.begin(C.byref(P[0])) == OK
    assert w.end(out.ctypes.data) == OK
    assert out.tobytes() == first
    assert set_plan() == OK                                          # a new plan empties both sets
    assert _dev_out(w, 0, 0) == STATE and _dev_out(w, 1, 0) == STATE
    assert _elapsed(w) == STATE
    return P, out, first


def test_channelizer(lib):
    words, bins = np.array([1 << 62], dtype=np.uint64), np.array([1], dtype=np.int32)
    with Walk(lib, 'channelizer', 'channelizer') as w:
        plan = lambda: w.set_plan(2, TAPS.ctypes.data, 3, words.ctypes.data, 1, 0, 1.0)                      # noqa: E731
        rational = lambda: w.set_plan_rational(1, 2, TAPS.ctypes.data, 3, words.ctypes.data, 1, 0, 1.0)      # noqa: E731
        uniform = lambda: w.set_plan_uniform(2, TAPS.ctypes.data, 3, bins.ctypes.data, 1, 0, 1.0)            # noqa: E731
        survey = lambda: w.set_survey(4, 0, 4.0)                                                             # noqa: E731
        # a plan of the other kind and a survey are refused by the kind of handle, in flight or not
        _channelizer_walk(w, plan, [(uniform, STATE), (survey, STATE)], 16)
        assert rational() == OK and plan() == OK                     # (idle: either kind of a plain handle's plans)
        P = _lib.ChannelizerParams(in_base=0, out_base=0, in_count=16, out_count=4, input=0, buffer=0)
        assert w.begin(C.byref(P)) == OK
        assert rational() == STATE
        assert w.survey_begin(C.byref(P), 0) == STATE and w.survey_end(None, None, None, None) == STATE
        assert w.end(None) == OK


def test_channelizer_uniform(lib):
    words, bins = np.array([1 << 62], dtype=np.uint64), np.array([1], dtype=np.int32)
    power, floor, mask = np.zeros(BINS, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint32)
    with Walk(lib, 'channelizer_uniform', 'channelizer') as w:
        plan = lambda: w.set_plan_uniform(2, TAPS.ctypes.data, 3, bins.ctypes.data, 1, 0, 1.0)               # noqa: E731
        plain = lambda: w.set_plan(2, TAPS.ctypes.data, 3, words.ctypes.data, 1, 0, 1.0)                     # noqa: E731
        assert w.set_survey(4, 0, 4.0) == STATE                      # no plan
        P, out, first = _channelizer_walk(w, plan, [(plain, STATE)], 64)
        # the survey: its own begin and end on the same busy flag
        assert w.survey_begin(C.byref(P[0]), 1) == STATE             # no survey set
        assert w.set_survey(4, 0, 4.0) == OK
        assert w.begin(C.byref(P[0])) == OK
        assert w.set_survey(4, 0, 4.0) == STATE                      # busy
        assert w.set_survey(3, 0, 4.0) == STATE                      # ... which comes before the argument error here
        assert w.survey_begin(C.byref(P[1]), 1) == STATE
        assert w.survey_end(None, None, None, None) == STATE         # a plain call ends with end
        assert w.end(None) == OK
        assert w.survey_begin(C.byref(P[1]), 0) == OK                # writes no output set
        assert w.end(None) == STATE                                  # a survey call ends with survey_end
        assert w.survey_end(out.ctypes.data, None, None, None) == ARG                # no outputs to copy: the call stays in flight
        assert _elapsed(w) == STATE
        assert w.survey_end(None, power.ctypes.data, floor.ctypes.data, mask.ctypes.data) == OK
        assert _elapsed(w) == OK
        assert _dev_out(w, 1, 0) == STATE and _dev_out(w, 0, 0) == OK        # the survey's set was not written
        assert power.sum() > 0
        assert w.survey_begin(C.byref(P[0]), 1) == OK
        out[:] = 0
        assert w.survey_end(out.ctypes.data, None, None, None) == OK
        assert out.tobytes() == first                                # the survey kernel's store is the plain kernel's
        assert w.set_survey(0, 0, 0.0) == OK                         # dropped
        assert w.survey_begin(C.byref(P[0]), 1) == STATE


def test_synthesizer(lib):
    out = np.zeros(5, np.complex64)
    P = [_lib.SynthesizerParams(out_base=0, out_count=5, buffer=b) for b in (0, 1)]
    place = _lib.SynthesizerPlacement(start=0, src=0, length=4, bin=1, gain=1.0)
    with Walk(lib, 'synthesizer', 'synthesizer') as w:
        begin = lambda b: w.begin(C.byref(P[b]), C.byref(place), 1)                  # noqa: E731
        plan = lambda: w.set_plan(2, TAPS.ctypes.data, 3)                            # noqa: E731
        source = lambda n=4: w.set_source(SOURCE.ctypes.data, n, 0)                  # noqa: E731
        assert w.end(None) == STATE
        assert source() == OK
        assert begin(0) == STATE                                     # a source, but no plan
        assert plan() == OK
        assert _elapsed(w) == STATE
    with Walk(lib, 'synthesizer', 'synthesizer') as w:
        assert plan() == OK
        assert begin(0) == STATE                                     # a plan, but no source
        assert w.begin(C.byref(P[0]), None, 0) == STATE              # ... which a call without placements needs too
        assert source() == OK
        assert _dev_out(w, 0) == STATE and _dev_out(w, 1) == STATE   # never written
        assert begin(0) == OK
        assert begin(0) == STATE
        assert plan() == STATE and source() == STATE
        assert source(5) == ARG and w.set_plan(2, TAPS.ctypes.data, 0) == ARG        # argument errors come first
        bad = _lib.SynthesizerParams(out_base=0, out_count=0, buffer=0)
        assert w.begin(C.byref(bad), C.byref(place), 1) == ARG
        assert _elapsed(w) == STATE                                  # busy, and before the first finished call
        assert _dev_out(w, 0) == STATE                               # in flight
        assert _dev_out(w, 1) == STATE                               # never written
        assert _dev_out(w, 2) == ARG
        assert w.end(out.ctypes.data) == OK
        first = out.tobytes()
        assert np.any(out != 0)
        assert w.end(None) == STATE
        assert _elapsed(w) == OK
        assert begin(1) == OK
        assert _dev_out(w, 0) == OK                                  # the other, finished set while a call is in flight
        assert _dev_out(w, 1) == STATE
        assert _elapsed(w) == STATE
        assert w.end(None) == OK                                     # clears busy
        assert _dev_out(w, 1) == OK
        out[:] = 0
        assert begin(0) == OK
        assert w.end(out.ctypes.data) == OK
        assert out.tobytes() == first
        assert plan() == OK                                          # a new plan empties both sets
        assert _dev_out(w, 0) == STATE and _dev_out(w, 1) == STATE
        assert _elapsed(w) == OK                                     # ... but the last call's time stays readable
