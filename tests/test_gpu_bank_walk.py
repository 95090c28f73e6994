"""A refusal and invalidation walk of the bank's block path, pinned on the library as it stood BEFORE its host side was split into
parts (profiles/bank_split.md): the file ran unmodified against that build (MFBANK_LIB) and against the split one.  It states what the
library answers, in the order of its checks -- not what anyone thinks it should answer.

1. The three ``_end`` entries: an idle slot, a slot that holds the other kind of flight, null result arrays (an argument error comes
   before the state test), a missing ``bands_c64`` and a record capacity one byte short -- both leave the flight in flight, and it is
   collected afterwards with the same numbers.
2. The setters that wait and invalidate the recorded graphs, while a flight is active: which refuse a single block, which a batch only.
3. Graph invalidation for the setters tests/test_gpu_block.py::test_block_graph_follows_changes_of_shifts_filters_and_tuning does not
   reach: flights with identical parameters until the graph has been recorded and replayed, the setter, the same again; every result
   after the change equals the result of a fresh handle configured that way from the start.  Compared, bit for bit, is every byte a
   batch of that kind writes: the scalars but ``clip_tag`` / ``clip_count`` (clipped fixed-shift batches only), ``sync_*`` (templates only)
   and ``a13_*`` (stages only); ``sym`` / ``cen`` / ``mag`` up to the block's count; the SNR windows up to their lengths (or the two means);
   with the stages on, bits / centres / trust up to ``a13_nwin`` and the tails up to their lengths.  The bytes behind those counts, and
   the fields named, hold whatever the allocation held on either handle (include/mfbank.h).  That the record has the layout of the
   setting in force -- no stage region behind the core after the stages went off -- is held by its size: the records' strides are equal.

The handle is the smallest one tests/test_gpu_block.py::test_block_calls_refuse_misuse builds (2^12 samples, 4 bins, 2 filters), with
filters of a short impulse response so that batches run (tests/test_gpu_sample_format.py::_bank).  Every call here is one a caller may make."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd._lib import MFB_ERR_ARG, MFB_ERR_STATE, MFB_OK
from pycusdr_amd.mfbank import BatchRecord, _ptr
from test_gpu_sample_format import K, N, _bank, _expect, _record_equal, _same_block

pytestmark = pytest.mark.gpu

OV = 1024
STRIDE = N - OV
B = 2
NWIN = B * STRIDE + OV
SC16 = 2.0 ** -15


def _stream(n, seed):
    """Noise, a tone and a few interference bursts (the clip has something to do), as int16 (I, Q) rows below full scale."""
    rng = np.random.default_rng(seed)
    x = 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.5 * np.exp(2j * np.pi * (1.3 / N) * np.arange(n))
    for p in rng.integers(0, n - 40, 6 * (n // N + 1)):
        x[p:p + int(rng.integers(1, 40))] *= rng.uniform(3, 8)
    q = np.round(np.stack((x.real, x.imag), axis=1) * (32000 / np.abs(np.stack((x.real, x.imag))).max()))
    return q.astype(np.int16)


def _arrays(bank, nb=1):
    cap = N // 2
    return (np.zeros(nb * cap, np.int32), np.zeros(nb * cap, np.int32), np.zeros(nb * cap, np.float32),
            np.zeros((nb, 2, bank.BAND_CAPACITY), np.complex64))


@pytest.fixture()
def bank():
    b = _bank()
    yield b
    b.close()


def _in_flight(bank):
    """A flight is active in some slot.  mfb_get_peak_clip_tail says so and, with the clip off, does nothing else: no wait, no epoch."""
    valid = C.c_int32(-1)
    rc = bank._lib.mfb_get_peak_clip_tail(bank._h, None, 0, C.byref(valid))
    assert rc in (MFB_OK, MFB_ERR_STATE) and (rc == MFB_ERR_STATE or valid.value == 0)
    return rc == MFB_ERR_STATE


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
def test_end_entries_refuse_in_the_order_of_their_checks(bank):
    lib, h = bank._lib, bank._h
    R, Rs, lay = _lib.BlockResult(), (_lib.BlockResult * B)(), _lib.RecordLayout()
    sym, cen, mag, bands = _arrays(bank, B)
    buf = np.zeros(1 << 18, np.uint8)
    cap = N // 2

    def end1(slot, r=R, s=sym, b=bands):
        return lib.mfb_receive_block_end(h, slot, C.byref(r) if r is not None else None, _ptr(s) if s is not None else None, _ptr(cen),
                                         _ptr(mag), _ptr(b) if b is not None else None)

    def endn(slot, r=Rs, s=sym, stride=cap, b=bands):
        return lib.mfb_receive_blocks_end(h, slot, r, _ptr(s) if s is not None else None, _ptr(cen), _ptr(mag), stride,
                                          _ptr(b) if b is not None else None)

    def endr(slot, dst=buf, capacity=None, layout=lay):
        return lib.mfb_receive_blocks_end_record(h, slot, _ptr(dst) if dst is not None else None, buf.size if capacity is None else capacity,
                                                 C.byref(layout) if layout is not None else None)

    # an idle slot; an argument error comes before the state test
    for slot in (0, 1):
        assert (end1(slot), endn(slot), endr(slot)) == (MFB_ERR_STATE,) * 3
        assert (end1(slot, r=None), end1(slot, s=None), endn(slot, r=None), endn(slot, s=None), endn(slot, stride=0), endr(slot, dst=None),
                endr(slot, layout=None)) == (MFB_ERR_ARG,) * 7
        assert (end1(slot, b=None), endn(slot, b=None)) == (MFB_ERR_STATE,) * 2        # (the bands are asked for by the flight: none here)
    assert (end1(2), endn(-1), endr(2)) == (MFB_ERR_ARG,) * 3

    # what the flights below must deliver: the same block and the same batch, collected the plain way
    q = _stream(NWIN, 3)
    x = _expect(q, SC16)
    bank.input[:] = x[:N]
    want1 = bank.receive_block(**K)
    win = bank.windows(B, STRIDE)
    win[1][:] = x
    bank.begin_blocks(1, B, source='window2', **K)
    wantB = bank.end_blocks_record(1)
    assert wantB.nb == B and not _in_flight(bank)

    # a single block in slot 0
    bank.begin_block(0, **K)
    assert (endn(0), endr(0)) == (MFB_ERR_STATE,) * 2 and _in_flight(bank)         # the other kind of flight
    assert end1(0, b=None) == MFB_ERR_ARG and _in_flight(bank)                     # searched with a band capacity: the bands are needed
    assert end1(0, s=None) == MFB_ERR_ARG and end1(0, r=None) == MFB_ERR_ARG and _in_flight(bank)
    assert end1(1) == MFB_ERR_STATE                                                # (the other slot is idle)
    assert end1(0) == MFB_OK and not _in_flight(bank)
    bank._blk = (sym[:cap], cen[:cap], mag[:cap], bands[0])
    _same_block(bank._block_result(R, True), want1, 'single block after refusals')
    bank._blk = None
    assert end1(0) == MFB_ERR_STATE

    # a batch in slot 1, collected with mfb_receive_blocks_end
    bank.begin_blocks(1, B, source='window2', **K)
    assert end1(1) == MFB_ERR_STATE and _in_flight(bank)                           # the other kind of flight
    assert endn(1, b=None) == MFB_ERR_ARG and endn(1, r=None) == MFB_ERR_ARG and endn(1, stride=0) == MFB_ERR_ARG and _in_flight(bank)
    assert endn(0) == MFB_ERR_STATE
    assert endn(1) == MFB_OK and not _in_flight(bank)
    for b in range(B):
        w = wantB.block(b)
        n = Rs[b].count
        assert n == len(w['symbols']) > 0 and Rs[b].shift == w['shift'] and Rs[b].spSym == w['spSym'] and Rs[b].codeOffset == w['codeOffset']
        assert np.float32(Rs[b].pick[0]) == w['pick'][0] and np.float32(Rs[b].pick[1]) == w['pick'][1]
        at = b * cap
        assert np.array_equal(sym[at:at + n], w['symbols']) and np.array_equal(cen[at:at + n], w['centres'])
        assert np.array_equal(mag[at:at + n].view(np.uint32), w['magnitudes'].view(np.uint32))
        for i in (0, 1):
            assert np.array_equal(bands[b, i, :Rs[b].band_len[i]].view(np.uint32), w['bands'][i].view(np.uint32))
    assert endn(1) == MFB_ERR_STATE

    # the batch again, collected as a record: a capacity one byte short says what is needed and leaves the batch in flight
    bank.begin_blocks(1, B, source='window2', **K)
    assert endr(1, capacity=1) == MFB_ERR_ARG and lay.nblocks == B and lay.record_bytes > 0 and _in_flight(bank)
    need = lay.nblocks * lay.record_bytes
    assert need <= buf.size
    lay.nblocks = lay.record_bytes = 0
    assert endr(1, capacity=need - 1) == MFB_ERR_ARG and (lay.nblocks, lay.record_bytes) == (B, need // B) and _in_flight(bank)
    assert lay.symbols == 0 and lay.off_sym == 0                                   # (nothing else of the layout is filled in)
    assert endr(1, capacity=need) == MFB_OK and not _in_flight(bank)
    _record_equal(BatchRecord(buf, lay, True), wantB, 'record after a short capacity')
    assert endr(1, capacity=need) == MFB_ERR_STATE


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
def test_setters_refuse_while_a_flight_is_active(bank):
    lib, h = bank._lib, bank._h
    fp = C.POINTER(C.c_float)()
    x = _expect(_stream(NWIN, 4), SC16)
    bank.input[:] = x[:N]
    want1 = bank.receive_block(**K)
    win = bank.windows(B, STRIDE)
    win[0][:] = x
    bank.begin_blocks(0, B, source='window', **K)
    wantB = bank.end_blocks_record(0)

    def every_flight():
        return (lib.mfb_set_peak_clip(h, C.c_float(4.5), 0), lib.mfb_set_peak_clip(h, C.c_float(0.0), 0), lib.mfb_set_device_snr(h, 1),
                lib.mfb_set_device_snr(h, 0), lib.mfb_set_sample_format(h, 1, C.c_float(0.0)), lib.mfb_set_sample_format(h, 0, C.c_float(0.0)))

    def batches_only():
        return (lib.mfb_set_batch_overlap(h, 1), lib.mfb_set_batch_overlap(h, 0), lib.mfb_window_buffer(h, 0, B + 1, STRIDE, C.byref(fp)),
                lib.mfb_window_buffer(h, 0, B, STRIDE, C.byref(fp)))

    # a single block in flight: the first three refuse -- whether or not the call would change anything -- the other two accept
    bank.begin_block(1, **K)
    assert every_flight() == (MFB_ERR_STATE,) * 6
    assert batches_only() == (MFB_OK,) * 4
    _same_block(bank.end_block(1), want1, 'single block beside the setters')
    assert every_flight() == (MFB_OK,) * 6 and batches_only() == (MFB_OK,) * 4

    # a batch in flight: all five refuse; asking for the windows as they are is no change and passes
    bank._win_key = None
    win = bank.windows(B, STRIDE)
    win[0][:] = x
    bank.begin_blocks(0, B, source='window', **K)
    assert every_flight() == (MFB_ERR_STATE,) * 6
    assert batches_only() == (MFB_ERR_STATE, MFB_ERR_STATE, MFB_ERR_STATE, MFB_OK)
    _record_equal(bank.end_blocks_record(0), wantB, 'batch beside the setters')
    assert every_flight() == (MFB_OK,) * 6


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
STAGES = dict(overlap_samples=OV, overlap_offset=20, match_threshold=10, error_threshold=1000, bit_lut=np.array([0, 1], np.uint8))
OFF = dict(overlap_samples=0, overlap_offset=0, match_threshold=0, error_threshold=0)
# name -> (configuration before, the setter, sample format before / after)
CHANGES = {
    'device_snr_on': ([], ('set_device_snr', (True,), {})),
    'device_snr_off': ([('set_device_snr', (True,), {})], ('set_device_snr', (False,), {})),
    'batch_overlap_on': ([], ('set_batch_overlap', (True,), {})),
    'batch_overlap_off': ([('set_batch_overlap', (True,), {})], ('set_batch_overlap', (False,), {})),
    'peak_clip_on': ([], ('set_peak_clip', (4.5, 0), {})),
    'peak_clip_scale': ([('set_peak_clip', (4.5, 0), {})], ('set_peak_clip', (3.0, 0), {})),
    'peak_clip_overlap': ([('set_peak_clip', (4.5, 0), {})], ('set_peak_clip', (4.5, OV // 2), {})),
    'sample_format': ([], ('set_sample_format', ('sc16',), {})),
    'stream_stages_on': ([], ('set_stream_stages', (), STAGES)),
    'stream_stages_off': ([('set_stream_stages', (), STAGES)], ('set_stream_stages', (), OFF)),
}


def _apply(bank, calls):
    for name, args, kw in calls:
        getattr(bank, name)(*args, **kw)


def _fill(bank, buf, q):
    buf[:] = q if bank.sample_format[0] == 'sc16' else _expect(q, SC16)


def _one_batch(bank, q):
    """One batch of B blocks in slot 0 from window 0, from a restarted clip chain and an empty stream tail."""
    _fill(bank, bank.windows(B, STRIDE)[0], q)
    bank.restart_peak_clip()
    if getattr(bank, '_stages', False):
        bank.stream_seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    bank.begin_blocks(0, B, source='window', **K)
    return bank.end_blocks_record(0)


def _one_block(bank, q):
    _fill(bank, bank.input, q[:N])
    bank.restart_peak_clip()
    bank.begin_block(0, **K)
    return bank.end_block(0)


# a batch's graph is kept per carry parity, which the stream stages flip with every batch: six batches replay each parity's once
REPS = 6


@pytest.mark.parametrize('change', sorted(CHANGES))
def test_recorded_graphs_follow_the_setters(change):
    before, setter = CHANGES[change]
    streams = [_stream(NWIN, 40 + i) for i in range(2 * REPS)]
    a, fresh = _bank(), _bank()
    try:
        _apply(a, before)
        for q in streams[:REPS]:             # plain launches, the recording, replays
            _one_batch(a, q)
        for q in streams[:3]:
            _one_block(a, q)
        _apply(a, [setter])
        _apply(fresh, before[:0] if change.endswith('_off') else before)
        _apply(fresh, [setter])
        if change.startswith('peak_clip'):
            assert sum(len(c) for c in _one_batch(fresh, streams[0]).clipped) > 0        # (the clip has something to do on this data)
        for i, q in enumerate(streams[REPS:]):
            Ra, Rf = _one_batch(a, q), _one_batch(fresh, q)
            assert Ra.stages == (change == 'stream_stages_on') and (Ra.snr_means is not None) == (change == 'device_snr_on'), (change, i)
            assert Ra.sym.strides == Rf.sym.strides and Ra.sym.shape == Rf.sym.shape, (change, i)        # (record bytes, symbols)
            _record_equal(Ra, Rf, (change, 'batch', i))
            if Ra.clipped is not None:
                for b in range(B):
                    assert np.array_equal(Ra.clipped[b], Rf.clipped[b]), (change, i, b)
        for i, q in enumerate(streams[REPS:REPS + 3]):
            _same_block(_one_block(a, q), _one_block(fresh, q), (change, 'block', i))
    finally:
        a.close()
        fresh.close()
