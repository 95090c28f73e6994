"""Integer IQ samples (``"HIP": {"sample_format": "sc16" | "sc8"}``), the parts that need no device: the configuration's
validation, the window assembler on (samples, 2) integer windows against the same assembler on complex64, the runner's dtype
checks over the CPU oracle bank, and the binding of the five new calls."""
import copy
import ctypes

import numpy as np
import pytest

import pycusdr_amd.demodulator.demodulator_base as dbm
from pycusdr_amd import _lib, config as cfg
from pycusdr_amd.demodulator.demodulator_base import as_samples, sample_format_config
from pycusdr_amd.demodulator_process import DemodulatorRunner
from pycusdr_amd.protocol import loadProtocol
from pycusdr_amd.sigFIFO import RingBuffer, WindowAssembler

from oracle_bank import OracleBank

NEW_CALLS = ('mfb_set_sample_format', 'mfb_get_sample_format', 'mfb_input_buffer_raw', 'mfb_window_buffer_raw', 'mfb_debug_unpack')


# ---- configuration ---------------------------------------------------------------------------------------------------------------
def test_accepted_forms_and_default_scales():
    assert sample_format_config({}, 'UHF') == (0, np.dtype(np.complex64), 1.0)
    assert sample_format_config({'sample_format': 'cf32'}, 'STX') == (0, np.dtype(np.complex64), 1.0)
    assert sample_format_config({'sample_format': 'sc16'}, 'UHF') == (1, np.dtype(np.int16), 2.0 ** -15)
    assert sample_format_config({'sample_format': 'sc8'}, 'UHF') == (2, np.dtype(np.int8), 2.0 ** -7)
    assert sample_format_config({'sample_format': 'sc16', 'sample_scale': 2.0 ** -11}, 'UHF') == (1, np.dtype(np.int16), 2.0 ** -11)
    assert sample_format_config({'sample_format': 'sc8', 'sample_scale': 8}, 'UHF') == (2, np.dtype(np.int8), 8.0)
    # the S-band back end with the clip on the device
    assert sample_format_config({'sample_format': 'sc16', 'device_clip': True}, 'STX')[0] == 1


@pytest.mark.parametrize('scale', [0.3, 0, -0.5, float('inf'), float('nan'), 3, 2.0 ** -140, 2.0 ** 125, 'x'])
def test_scales_that_are_no_power_of_two_are_refused(scale):
    for fmt in ('sc16', 'sc8'):
        with pytest.raises(ValueError):
            sample_format_config({'sample_format': fmt, 'sample_scale': scale}, 'UHF')


def test_refusals():
    for name in ('sc12', 'int16', '', None, 16):
        with pytest.raises(ValueError):
            sample_format_config({'sample_format': name}, 'UHF')
    with pytest.raises(ValueError):          # sharding moves complex64 tensors
        sample_format_config({'sample_format': 'sc16'}, 'UHF', shard=object())
    assert sample_format_config({}, 'UHF', shard=object())[0] == 0
    for backend in ('STX', 'STX1', None):    # the host's clip writes floats back into the samples
        with pytest.raises(ValueError):
            sample_format_config({'sample_format': 'sc8'}, backend)
        with pytest.raises(ValueError):
            sample_format_config({'sample_format': 'sc8', 'device_clip': False}, backend)
        with pytest.raises(ValueError):      # the device clip runs on the one-call path only
            sample_format_config({'sample_format': 'sc8', 'device_clip': True, 'one_call': False}, backend)
    with pytest.raises(ValueError):
        sample_format_config({'sample_format': 'cf32', 'sample_scale': 0.5}, 'UHF')


def test_as_samples_takes_views_and_refuses_other_dtypes():
    flat = np.arange(20, dtype=np.int16)
    v = as_samples(flat, np.int16)
    assert v.shape == (10, 2) and np.shares_memory(v, flat)
    pairs = flat.reshape(10, 2)
    assert as_samples(pairs, np.int16) is pairs
    for bad in (flat.astype(np.complex64), flat.astype(np.int8), flat.astype(np.int32), flat.astype(np.float32)):
        with pytest.raises(TypeError):
            as_samples(bad, np.int16)
    with pytest.raises(ValueError):
        as_samples(flat[:5], np.int16)
    with pytest.raises(ValueError):
        as_samples(flat.reshape(5, 4), np.int16)


# ---- the window assembler on integer windows ---------------------------------------------------------------------------------------
N, OV, B = 4096, 1021, 3
STRIDE = N - OV


def _deq(a, scale):
    return np.ascontiguousarray(a.astype(np.float32) * np.float32(scale)).view(np.complex64).reshape(len(a))


@pytest.mark.parametrize('dtype,scale', [(np.int16, 2.0 ** -11), (np.int8, 2.0 ** -7)])
def test_window_assembler_on_integer_windows_equals_complex64(dtype, scale):
    rng = np.random.default_rng(5)
    info = np.iinfo(dtype)
    nwin = B * STRIDE + OV
    stream = rng.integers(info.min, info.max + 1, size=(5 * B * STRIDE + 777, 2)).astype(dtype)
    wi = [np.zeros((nwin, 2), dtype), np.zeros((nwin, 2), dtype)]
    wc = [np.zeros(nwin, np.complex64), np.zeros(nwin, np.complex64)]
    wi[0][:OV] = stream[:OV]
    wc[0][:OV] = _deq(stream[:OV], scale)
    ai, ac = WindowAssembler(wi[0], OV, STRIDE, B), WindowAssembler(wc[0], OV, STRIDE, B)
    cur, pos, taken = 0, OV, 0
    # chunk lengths that straddle two windows (a chunk is cut where a window is full), tiny ones, one of several windows' worth
    lengths = [5000, 1, 4095, 7000, 3, 9225, 2 * nwin + 11, 123, 6000, 5000, 8191]
    k = 0
    while pos < len(stream):
        ln = lengths[k % len(lengths)]
        k += 1
        chunk = stream[pos:pos + ln]
        pos += len(chunk)
        rest_i, rest_c = chunk, _deq(chunk, scale)
        while len(rest_i):
            ni, nc = ai.take(rest_i), ac.take(rest_c)
            assert ni == nc
            rest_i, rest_c = rest_i[ni:], rest_c[nc:]
            assert ai.fill == ac.fill and ai.full() == ac.full() and ai.complete_blocks() == ac.complete_blocks()
            assert len(ai.stamps) == len(ac.stamps) == ai.complete_blocks()
            assert np.array_equal(_deq(ai.buf[:ai.fill], scale), ac.buf[:ac.fill])
            if ai.full() or (k % 4 == 0 and ai.complete_blocks()):
                nb = ai.complete_blocks()          # a whole window, or -- now and then -- the complete blocks of a partly filled one
                taken += nb
                # the window holds the stream: block b of this window is samples [first + b * stride, ... + N)
                first = (taken - nb) * STRIDE
                assert np.array_equal(ai.buf[:nb * STRIDE + OV], stream[first:first + nb * STRIDE + OV])
                cur = 1 - cur
                ai.retarget(wi[cur], nb)
                ac.retarget(wc[cur], nb)
                assert ai.fill == ac.fill and len(ai.stamps) == len(ac.stamps)
                assert np.array_equal(_deq(ai.buf[:ai.fill], scale), ac.buf[:ac.fill])      # the carried overlap (and what follows)
                assert np.array_equal(ai.buf[:OV], stream[taken * STRIDE:taken * STRIDE + OV])
    assert taken >= 4 * B
    with pytest.raises(IndexError):
        WindowAssembler(np.zeros((nwin - 1, 2), dtype), OV, STRIDE, B)


def test_ring_buffer_of_integer_pairs():
    r = RingBuffer(6, bufLen=10, dtype=np.int16, row=(2,))
    a = np.arange(16, dtype=np.int16).reshape(8, 2)
    assert r.insert(a) == 8
    assert np.array_equal(r.popBlock(6), a[:6])
    assert r.insert(a[:7]) == 9                         # wraps around the end of the store
    assert np.array_equal(r.popBlock(6), np.concatenate((a[6:], a[:4])))


# ---- the runner's dtype checks, over the CPU oracle bank ------------------------------------------------------------------------------
class IntegerOracleBank(OracleBank):
    """OracleBank with the sample-format call of MFBank: ``input`` becomes an (N, 2) integer buffer, dequantised on upload."""
    fmt_scale = None

    def set_sample_format(self, fmt, scale=None):
        dt = {'sc16': np.int16, 'sc8': np.int8}[fmt]
        self.fmt_scale = scale if scale is not None else {'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}[fmt]
        self.input = np.zeros((self.N, 2), dt)

    def upload(self, samples=None):
        assert samples is None or self.fmt_scale is None
        if self.fmt_scale is None:
            return OracleBank.upload(self, samples)
        OracleBank.upload(self, (self.input.astype(np.float32) * np.float32(self.fmt_scale)).view(np.complex64).reshape(self.N))


@pytest.fixture()
def oracle_backend(monkeypatch):
    monkeypatch.setattr(dbm, 'MFBank', IntegerOracleBank)


def _conf(fmt=None, **hip):
    conf = copy.deepcopy(cfg.bench_config('bench_GMSK', blockSize=12, doppCarrierSteps=4))
    if fmt is not None:
        conf['GPU']['UHF'].setdefault('HIP', {}).update(sample_format=fmt, **hip)
    return conf


def test_runner_takes_integer_chunks_as_views_and_refuses_other_dtypes(oracle_backend):
    conf = _conf('sc16', sample_scale=2.0 ** -11)
    p = loadProtocol('bench_GMSK')(conf=conf)
    run = DemodulatorRunner(conf, p, 'UHF-H')
    ref = DemodulatorRunner(_conf(), p, 'UHF-H')
    try:
        assert run.dtype == np.int16 and run.raw.dtype == np.int16 and run.raw.shape == (run.blockSize, 2)
        assert ref.dtype == np.complex64 and ref.raw.shape == (ref.blockSize,)
        n = run.samplesPerSlice
        rng = np.random.default_rng(1)
        q = rng.integers(-2000, 2000, size=(n, 2)).astype(np.int16)
        for bad in (_deq(q, 2.0 ** -11), q.astype(np.int8), q.astype(np.int32), q.astype(np.float32)):
            for call in (run.feed, run.feed_device, run.feed_device_begin, run.skip_block):
                with pytest.raises(TypeError):
                    call(bad)
            with pytest.raises(TypeError):
                run.run([bad])
            with pytest.raises(TypeError):
                run.run_stream([bad])
            with pytest.raises(TypeError):
                run.run_stream([bad], pipelined=True)
        assert run.count == 0 and not run.raw.any()        # nothing of a refused chunk went anywhere
        # (n, 2) and flat 2n give the same block as the complex64 runner fed the dequantised samples
        flat = q.reshape(-1)
        assert flat.base is q or flat.base is q.base
        a = run.feed(flat)
        assert np.array_equal(run.raw[:run.overlap], q[-run.overlap:])
        b = ref.feed(_deq(q, 2.0 ** -11))
        q2 = rng.integers(-2000, 2000, size=(n, 2)).astype(np.int16)
        a2, b2 = run.feed(q2), ref.feed(_deq(q2, 2.0 ** -11))
        for x, y in ((a, b), (a2, b2)):
            for k in ('count', 'doppler', 'SNR', 'spSymEst'):
                assert np.array_equal(x[k], y[k], equal_nan=True), k
            assert np.array_equal(x['data'], y['data']) and np.array_equal(x['trust'], y['trust'])
        # the stream forms: chunks of any size, flat or paired
        s = rng.integers(-2000, 2000, size=(3 * n, 2)).astype(np.int16)
        ra, _ = run.run_stream([s[:5000].reshape(-1), s[5000:]])
        rb, _ = ref.run_stream([_deq(s, 2.0 ** -11)])
        rc, _ = run.run_stream([s[:777], s[777:].reshape(-1)], pipelined=True)
        assert len(ra) == len(rb) == len(rc) == 3
        run.skip_block(q)
        assert np.array_equal(run.raw[:run.overlap], q[-run.overlap:])
        # the host-clip entry points refuse integer samples
        with pytest.raises(TypeError):
            run.demod.thresholdInput(run.raw)
        with pytest.raises(TypeError):
            run.demod.uploadAndFindUHF(run.raw)
    finally:
        run.close()
        ref.close()


def test_demodulator_refuses_bad_sample_formats_before_it_touches_the_device(oracle_backend):
    from pycusdr_amd.demodulator import UHF
    for hip in ({'sample_format': 'sc12'}, {'sample_format': 'sc16', 'sample_scale': 0.3}):
        conf = _conf()
        conf['GPU']['UHF']['HIP'] = hip
        with pytest.raises(ValueError):
            UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')


# ---- binding ---------------------------------------------------------------------------------------------------------------------
def test_the_new_calls_are_bound_and_exported():
    import __graft_entry__
    lib = ctypes.CDLL(__graft_entry__.build())
    for name in NEW_CALLS:
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert _lib.load().mfb_abi_version() == 9            # additive: found by symbol, the version stays
    # argument checks that need no device
    assert _lib.load().mfb_debug_unpack(0, 0, 0.0, None, 1, None) == _lib.MFB_ERR_ARG
    assert _lib.load().mfb_set_sample_format(None, 1, 0.0) == _lib.MFB_ERR_ARG


def test_host_copy_counts_rows_of_integer_windows():
    """The copy worker moves bytes: offsets and lengths are rows of the window, 4 bytes each for sc16 -- not 8."""
    from pycusdr_amd.mfbank import HostCopy
    hc = HostCopy()
    try:
        for dtype in (np.int16, np.int8):
            nwin = B * STRIDE + OV
            win = np.zeros((nwin, 2), dtype)
            src = (np.arange(2 * 5000) % 100).astype(dtype).reshape(5000, 2)
            src.flags.writeable = False                   # a read-only chunk: its copy is queued
            asm = WindowAssembler(win, OV, STRIDE, B, copier=hc)
            assert asm.take(src) == 5000
            hc.drain()
            assert np.array_equal(win[OV:OV + 5000], src) and not win[:OV].any() and not win[OV + 5000:].any()
        with pytest.raises(ValueError):
            hc.submit(win, 0, np.zeros(10, np.int8))      # flat samples into a window of pairs
        with pytest.raises(IndexError):
            hc.submit(win, nwin - 5, np.zeros((10, 2), np.int8))
    finally:
        hc.close()
