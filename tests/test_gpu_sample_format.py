"""Integer IQ samples converted on the device (mfb_set_sample_format, csrc/unpack_kernels.hpp): sc16 and sc8 in the page-locked
inputs must give, bit for bit, what a complex64 handle gives when it is fed the host's conversion of the same integers --
``(raw.astype(np.float32) * np.float32(scale)).view(np.complex64)`` -- through the kernel's test seam, one block, recorded graphs,
batches (with and without the stream stages), the peak clip, the calls' contract and the receive loop.  Everything is compared
as bits (uint32) or with array_equal: there is no tolerance, the conversion is exact."""
import copy

import numpy as np
import pytest

import clip_model as cm
from pycusdr_amd import _lib, config as cfg, signals as sg
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.demodulator_process import DemodulatorRunner
from pycusdr_amd.mfbank import MFBank, debug_unpack
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu

LOG2N, N = 12, 1 << 12
K = dict(k_offset=200, k_len=100, spsym_min=8)
DT = {'sc16': np.int16, 'sc8': np.int8}
STEP = {'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}       # the default value of one integer step


def _expect(raw, scale):
    return np.ascontiguousarray(raw.astype(np.float32) * np.float32(scale)).view(np.complex64).reshape(len(raw))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bank(seed=0, taps=32):
    """A search handle as tests/test_gpu_peak_clip.py builds its own: two filters with a short impulse response (segment path:
    batches run there), 4 shifts."""
    rs = np.random.RandomState(seed)
    h = np.zeros((2, N), np.complex64)
    h[:, :taps] = rs.standard_normal((2, taps)) + 1j * rs.standard_normal((2, taps))
    bank = MFBank(LOG2N, 4, 2)
    bank.set_filters(np.conj(np.fft.fft(h, axis=1)).astype(np.complex64))
    bank.set_shifts([0, 1, 2, 3])
    return bank


def _quantised(fmt, n, seed):
    """Noise plus a tone, quantised to the format: most of its range used, nothing clipped."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(DT[fmt]).max
    t = np.arange(n)
    x = 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.5 * np.exp(2j * np.pi * (1.3 / N) * t * (1 + seed % 3))
    q = np.round(np.stack((x.real, x.imag), axis=1) * (top / 1.6))
    assert np.abs(q).max() <= top
    return q.astype(DT[fmt])


def _same_block(a, b, tag=''):
    """Every field of two receive_block results."""
    assert set(a) == set(b), tag
    for k in a:
        if k == 'bands':
            assert (a[k] is None) == (b[k] is None), (tag, k)
            if a[k] is not None:
                for u, v in zip(a[k], b[k]):
                    assert np.array_equal(_bits(u), _bits(v)), (tag, k)
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (tag, k)
        elif isinstance(a[k], tuple):
            assert np.array_equal(_bits(np.array(a[k], np.float32)), _bits(np.array(b[k], np.float32))), (tag, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k, a[k], b[k])
    assert len(a['symbols']) > 0, tag


# ---- 1, 2: the kernel through its seam -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['sc16', 'sc8'])
def test_seam_every_value(fmt):
    info = np.iinfo(DT[fmt])
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    raw = np.stack((v, v[::-1]), axis=1).astype(DT[fmt])       # I runs through every value, Q through them reversed
    assert len(raw) == (65536 if fmt == 'sc16' else 256)
    for scale in (None, 2.0 ** -11, 2.0 ** 3):
        got = debug_unpack(raw, fmt, scale)
        want = _expect(raw, STEP[fmt] if scale is None else scale)
        assert np.array_equal(_bits(got), _bits(want)), (fmt, scale)


@pytest.mark.parametrize('fmt', ['sc16', 'sc8'])
def test_seam_tails_and_nothing_written_behind_the_last_sample(fmt):
    rng = np.random.default_rng(7)
    info = np.iinfo(DT[fmt])
    sentinel = np.complex64(complex(-1234.5, 6789.25))
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4099):
        raw = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(DT[fmt])
        out = np.full(n + 1, sentinel, np.complex64)
        debug_unpack(raw, fmt, 2.0 ** -11, out=out)
        assert np.array_equal(_bits(out[:n]), _bits(_expect(raw, 2.0 ** -11))), (fmt, n)
        assert _bits(out[n:]).tolist() == _bits(np.array([sentinel])).tolist(), (fmt, n)


# ---- 3, 4: one block ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def pair():
    a, b = _bank(), _bank()
    yield a, b
    a.close()
    b.close()


def _want_block(plain, x):
    plain.input[:] = x
    r = plain.receive_block(**K)
    return r, plain.get_spectrum(0, N)


def _check_one_block(a, plain, fmt, scale, seed):
    """The handle ``a`` (format ``fmt`` in force) on one quantised block, every way in, against the complex64 handle."""
    q = _quantised(fmt, N, seed)
    want, wantX = _want_block(plain, _expect(q, STEP[fmt] if scale is None else scale))
    assert a.input.dtype == DT[fmt] and a.input.shape == (N, 2)
    a.input[:] = q
    _same_block(a.receive_block(**K), want, (fmt, 'pinned'))
    assert np.array_equal(_bits(a.get_spectrum(0, N)), _bits(wantX))
    a.upload()                                        # mfb_upload: the pinned buffer, on the handle's stream
    assert np.array_equal(_bits(a.get_spectrum(0, N)), _bits(wantX))
    assert a.input2.dtype == DT[fmt] and a.input2.shape == (N, 2)
    a.input2[:] = q
    a.input[:] = 0
    for slot, source in ((0, 'pinned2'), (1, 'pinned2')):
        a.begin_block(slot, source=source, **K)
        _same_block(a.end_block(slot), want, (fmt, slot, source))
    a.input[:] = q
    a.begin_block(1, source='pinned', **K)
    _same_block(a.end_block(1), want, (fmt, 1, 'pinned'))
    assert np.array_equal(_bits(a.get_spectrum(0, N)), _bits(wantX))
    assert np.array_equal(a.input, q)                 # the caller's samples stay as they were


@pytest.mark.parametrize('fmt,scale', [('sc16', None), ('sc16', 2.0 ** -11), ('sc8', None), ('sc8', 2.0 ** 3)])
def test_one_block_equals_the_complex64_handle(pair, fmt, scale):
    a, plain = pair
    a.set_sample_format(fmt, scale)
    name, dtype, step, nbytes = a.sample_format
    assert (name, dtype, step, nbytes) == (fmt, np.dtype(DT[fmt]), STEP[fmt] if scale is None else scale, 4 if fmt == 'sc16' else 2)
    _check_one_block(a, plain, fmt, scale, seed=3)


def test_graph_replay_follows_the_data(pair):
    """The same slot three times: plain launches, the capture, the replay -- the copy and the conversion stay outside the graph, so
    each block is its own."""
    a, plain = pair
    a.set_sample_format('sc16')
    for rounds, source in ((3, 'pinned'), (4, 'pinned2')):
        buf = a.input if source == 'pinned' else a.input2
        for i in range(rounds):
            q = _quantised('sc16', N, 10 + i)
            want, _ = _want_block(plain, _expect(q, STEP['sc16']))
            buf[:] = q
            a.begin_block(0, source=source, **K)
            _same_block(a.end_block(0), want, (source, i))


# ---- 5: batches --------------------------------------------------------------------------------------------------------------------
OV, B = 1021, 3
STRIDE = N - OV
NWIN = B * STRIDE + OV          # 10246 samples: a multiple of neither 4 nor 8 -- the kernel's tail runs in the product path


def _record_equal(Ra, Rb, tag):
    """Everything a finished batch hands out, block for block (what is valid of it: the counts say how much)."""
    assert Ra.nb == Rb.nb and Ra.stages == Rb.stages, tag
    # fields a batch of this kind does not write hold whatever an earlier flight left (include/mfbank.h): the clip tags outside
    # clipped fixed-shift batches, the stream stages' fields without the stages, the sync hits without templates
    def written(k):
        return not (k in ('clip_tag', 'clip_count') or k.startswith('sync_') or (k.startswith('a13_') and not Ra.stages))
    for k in Ra.s:
        if written(k):
            assert np.array_equal(np.array(Ra.s[k]), np.array(Rb.s[k]), equal_nan=True), (tag, k)
    for b in range(Ra.nb):
        _same_block(Ra.block(b), Rb.block(b), (tag, b))
        if Ra.stages and Ra.s['a13_status'][b]:
            nw = Ra.s['a13_nwin'][b]
            for name in ('bits', 'cen8', 'trust'):
                assert np.array_equal(getattr(Ra, name)[b, :nw], getattr(Rb, name)[b, :nw]), (tag, b, name)
            assert np.array_equal(Ra.post[b, :Ra.s['a13_npost'][b]], Rb.post[b, :Rb.s['a13_npost'][b]]), (tag, b)
            assert np.array_equal(Ra.end[b, :Ra.s['a13_nend'][b]], Rb.end[b, :Rb.s['a13_nend'][b]]), (tag, b)


@pytest.mark.parametrize('stages', [False, True])
@pytest.mark.parametrize('fmt', ['sc16', 'sc8'])
def test_batches_equal_the_complex64_handle(pair, fmt, stages):
    assert NWIN == 10246 and NWIN % 4 and NWIN % 8
    a, plain = pair
    a.set_sample_format(fmt)
    if stages:
        # the bank-level form of Demodulator.enableStreamStages / seedStreamStages (tests/test_gpu_stream_stages.py): a 0 / 1 bit LUT
        # over the two filters, the alignment's thresholds, an empty tail to start from
        for h in (a, plain):
            h.set_stream_stages(1024, 20, 10, 1000, bit_lut=np.array([0, 1], np.uint8))
            h.stream_seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    wa, wp = a.windows(B, STRIDE), plain.windows(B, STRIDE)
    assert all(w.dtype == DT[fmt] and w.shape == (NWIN, 2) for w in wa) and all(w.shape == (NWIN,) for w in wp)
    stream = _quantised(fmt, 4 * B * STRIDE + OV, 21)
    names = ('window', 'window2')
    for turn in range(2):
        # both windows, both slots, two batches in flight
        for h, wins, conv in ((a, wa, lambda q: q), (plain, wp, lambda q: _expect(q, STEP[fmt]))):
            for i in (0, 1):
                first = (2 * turn + i) * B * STRIDE
                wins[i][:] = conv(stream[first:first + NWIN])
                h.begin_blocks(i, B if (turn, i) != (1, 1) else B - 1, source=names[i], **K)
        for i in (0, 1):
            _record_equal(a.end_blocks_record(i), plain.end_blocks_record(i), (fmt, stages, turn, i))
    # the scores of the batch begun last
    assert np.array_equal(_bits(a.get_batch_scores(0)), _bits(plain.get_batch_scores(0)))


# ---- 6: the peak clip on integer input ------------------------------------------------------------------------------------------------
def test_peak_clip_on_integer_input(pair):
    a, plain = pair
    rng = np.random.default_rng(4)
    ov = 1024
    stride = N - ov
    x = cm.bursty(rng, 4 * stride + ov, bursts=12)
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    gain = 2.0 ** np.floor(np.log2(32767 / peak))            # the bursts below full scale
    q = np.round(np.stack((x.real, x.imag), axis=1) * gain).astype(np.int16)
    assert np.abs(np.round(np.stack((x.real, x.imag), axis=1) * gain)).max() < 32767
    xs = _expect(q, 1.0 / gain)
    a.set_sample_format('sc16', 1.0 / gain)
    for h in (a, plain):
        h.set_peak_clip(4.5, ov)
    clipped = 0
    # one block, then a 3-block batch that continues it: the chain runs across the calls
    for h, first, conv in ((a, q, lambda v: v), (plain, xs, lambda v: v)):
        h.input[:] = first[:N]
    ra, rb = a.receive_block(fixed_shift=1, **K), plain.receive_block(fixed_shift=1, **K)
    _same_block(ra, rb, 'clip block')
    clipped += len(ra['clipped'])
    assert np.array_equal(_bits(a.get_spectrum(0, N)), _bits(plain.get_spectrum(0, N)))
    wa, wp = a.windows(3, stride), plain.windows(3, stride)
    wa[0][:] = q[stride:]
    wp[0][:] = xs[stride:]
    for h in (a, plain):
        h.begin_blocks(0, 3, fixed_shift=1, source='window', **K)
    Ra, Rb = a.end_blocks_record(0), plain.end_blocks_record(0)
    _record_equal(Ra, Rb, 'clip batch')
    for b in range(3):
        assert np.array_equal(Ra.clipped[b], Rb.clipped[b]), b
        clipped += len(Ra.clipped[b])
    assert clipped > 0
    ta, tb = a.peak_clip_tail(ov), plain.peak_clip_tail(ov)
    assert ta is not None and np.array_equal(_bits(ta), _bits(tb))


# ---- 7: the contract -----------------------------------------------------------------------------------------------------------------
def test_contract_and_refusals_leave_the_handle_working(pair):
    a, plain = pair
    a.set_sample_format('sc16')

    def still_works(fmt='sc16', scale=None):
        _check_one_block(a, plain, fmt, scale, seed=5)

    still_works()
    with pytest.raises(ValueError):
        a.set_sample_format('sc12')
    with pytest.raises(ValueError):
        _lib.check(a._lib.mfb_set_sample_format(a._h, 7, 0.0), 'mfb_set_sample_format')
    still_works()
    for bad in (0.3, -0.5, float('inf'), float('nan'), 2.0 ** 125, 2.0 ** -140):
        with pytest.raises(ValueError):
            a.set_sample_format('sc16', bad)
    assert a.sample_format[0] == 'sc16'
    still_works()
    a.input[:] = _quantised('sc16', N, 1)
    a.begin_block(0, source='pinned', **K)
    with pytest.raises(RuntimeError):                 # a flight is open
        a.set_sample_format('sc8')
    a.end_block(0)
    assert a.sample_format[0] == 'sc16'
    still_works()
    with pytest.raises(ValueError):                   # mfb_upload_from takes complex64: unsupported while the buffer holds integers
        a.upload(np.zeros(N, np.complex64))
    still_works()
    # the complex64 accessors refuse instead of handing out a mistyped pointer
    import ctypes as C
    buf = C.POINTER(C.c_float)()
    assert a._lib.mfb_input_buffer(a._h, C.byref(buf)) == _lib.MFB_ERR_STATE
    assert a._lib.mfb_input_buffer2(a._h, C.byref(buf)) == _lib.MFB_ERR_STATE
    assert a._lib.mfb_window_buffer(a._h, 0, 2, N - 64, C.byref(buf)) == _lib.MFB_ERR_STATE
    still_works()
    # sc16 -> cf32 -> sc8 on one handle
    a.set_sample_format('cf32')
    assert a.input.dtype == np.complex64 and a.input.shape == (N,) and a.sample_format[3] == 8
    assert not a.input.any()                          # a change zero-fills the buffers
    x = _expect(_quantised('sc16', N, 8), STEP['sc16'])
    want, wantX = _want_block(plain, x)
    a.input[:] = x
    _same_block(a.receive_block(**K), want, 'cf32 again')
    a.upload(x.copy())                                # ... and mfb_upload_from works again
    assert np.array_equal(_bits(a.get_spectrum(0, N)), _bits(wantX))
    a.set_sample_format('sc8', 2.0 ** -5)
    still_works('sc8', 2.0 ** -5)


# ---- 8: the receive loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bpc', [1, 4])
def test_receive_loop_on_int16_chunks_equals_complex64(bpc):
    bs, ov = 15, 1 << 10
    n = 1 << bs
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
    conf['GPU']['UHF'].setdefault('HIP', {})['blocks_per_call'] = bpc
    confI = copy.deepcopy(conf)
    confI['GPU']['UHF']['HIP'].update(sample_format='sc16', sample_scale=2.0 ** -11)
    p = loadProtocol('bench_GMSK')(conf=conf)
    nblocks = 9
    sig = sg.s1_stream(nblocks, n, ov, 'GMSK', snr_db=12.0, seed=3)[ov:]
    q = np.round(np.stack((sig.real, sig.imag), axis=1) * 2.0 ** 11)
    assert np.abs(q).max() < 32767
    q = q.astype(np.int16)
    x = _expect(q, 2.0 ** -11)
    q.flags.writeable = x.flags.writeable = False       # a recording: the batched loop queues its copies for the copy thread
    a, b = DemodulatorRunner(confI, p, 'UHF-H'), DemodulatorRunner(conf, p, 'UHF-H')
    try:
        assert a.raw.dtype == np.int16 and a.dtype == np.int16
        da, db = Decoder(conf, p), Decoder(conf, p)
        ra, pa = a.run_stream((q[i:i + 5000] for i in range(0, len(q), 5000)), decoder=da)
        rb, pb = b.run_stream((x[i:i + 5000] for i in range(0, len(x), 5000)), decoder=db)
        assert len(ra) == len(rb) == nblocks
        for u, v in zip(ra, rb):
            for k in ('count', 'doppler', 'SNR', 'spSymEst', 'numSyncSig'):
                assert np.array_equal(u[k], v[k], equal_nan=True), (u['count'], k)
            assert np.array_equal(u['data'], v['data']) and np.array_equal(u['trust'], v['trust']), u['count']
        assert len(pa) == len(pb) and all(np.array_equal(s.bits, t.bits) for s, t in zip(pa, pb))
        with pytest.raises(TypeError):                # never converted on this thread
            a.run_stream([x[:5000]])
    finally:
        a.close()
        b.close()
