"""The device-side SNR means (mfb_set_device_snr; reference computeSNR, demodulator/demodulator_base.py:635-667) as far as a machine
without a GPU can see them: the new symbols, the unchanged ABI version, and the config key ``"HIP": {"device_snr": true}`` on its way
through ``Demodulator.__init__`` to the handle (a fake bank, as tests/test_demod_hostlogic.py uses one)."""
import ctypes
import logging

import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.demodulator import UHF
from pycusdr_amd.demodulator.demodulator_base import Demodulator
from pycusdr_amd.protocol import loadProtocol
import pycusdr_amd.demodulator.demodulator_base as dbm

from oracle_bank import OracleBank


def test_library_has_the_new_symbols_and_the_old_version():
    import __graft_entry__
    lib = ctypes.CDLL(__graft_entry__.build())
    for name in ('mfb_set_device_snr', 'mfb_get_block_snr', 'mfb_debug_band_means'):
        assert hasattr(lib, name), name
    assert lib.mfb_abi_version() == 9
    # bad arguments are refused before any device is touched
    assert lib.mfb_set_device_snr(None, 1) == 1 and lib.mfb_get_block_snr(None, 0, 0, None, None) == 1
    assert lib.mfb_debug_band_means(0, None, 16, 1, None, None) == 1
    X = np.zeros(16, np.complex64)
    means = np.zeros(1, np.float32)
    for bad in ([[0, 17], [0, 0]], [[-1, 4], [0, 0]], [[0, 4], [14, 3]], [[0, 9], [0, 9]], [[0, 4], [0, -1]]):
        pieces = np.array([bad], np.int32)
        rc = lib.mfb_debug_band_means(0, X.ctypes.data_as(ctypes.c_void_p), 16, 1, pieces.ctypes.data_as(ctypes.c_void_p),
                                      means.ctypes.data_as(ctypes.c_void_p))
        assert rc == 1, bad                   # MFB_ERR_ARG: a piece outside [0, N]


class OneCallBank(OracleBank):
    """An OracleBank that claims the one-call block path and records what the constructor switches."""
    BAND_CAPACITY = 1024

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.device_snr_calls = []

    def receive_block(self, *a, **kw):
        raise AssertionError('no block is received in these tests')

    def set_device_snr(self, on=True):
        self.device_snr_calls.append(bool(on))


@pytest.fixture()
def fake_bank(monkeypatch):
    monkeypatch.setattr(dbm, 'MFBank', OneCallBank)


def _conf(key, **kw):
    conf = cfg.bench_config('bench_GMSK', blockSize=12, doppCarrierSteps=8, **kw)
    if key is not None:
        conf['GPU']['UHF']['HIP'] = {'device_snr': key}
    return conf


def test_config_key_reaches_the_handle(fake_bank):
    conf = _conf(True)
    d = UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')
    assert d.bank.device_snr_calls == [True] and d.bank.BAND_CAPACITY == 1 and d._device_snr
    for key in (None, False):
        conf = _conf(key)
        d = UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')
        assert d.bank.device_snr_calls == [] and d.bank.BAND_CAPACITY >= 256 and not d._device_snr


def test_key_with_a_shard_raises(fake_bank):
    conf = _conf(True)
    with pytest.raises(ValueError, match='device_snr'):
        UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H', shard=object())


def test_key_needs_the_one_call_path(fake_bank):
    conf = _conf(True)
    conf['GPU']['UHF']['HIP']['one_call'] = False
    with pytest.raises(ValueError, match='one-call'):
        UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')


def test_capacity_warning_only_without_the_key(fake_bank, caplog):
    """Two bins 2^17 spectrum bins apart at N = 2^18: a window of more than the 2^16 elements that travel with a block."""
    def build(key):
        conf = _conf(key, rangeRateMax=25000)
        conf['GPU']['UHF']['blockSize'] = 18
        conf['Radios']['Rx']['UHF-H']['doppCarrierSteps'] = 2
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger=dbm.log.name):
            d = UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')
        assert Demodulator._snr_band_capacity(d, 5)[1] > 1 << 16
        return [r for r in caplog.records if 'longer SNR window' in r.getMessage()]
    assert len(build(None)) == 1
    assert build(True) == []


def test_snr_from_means_is_computesnr_last_line():
    """The host formula on two delivered means: computeSNR's own operations (DB:662-667), float32 throughout, on scalars and per block."""
    rng = np.random.default_rng(0)
    sig = rng.uniform(0.5, 50, 64).astype(np.float32)
    noise = rng.uniform(0.5, 5, 64).astype(np.float32)
    sig[:3], noise[:3] = (0, 1, np.nan), (0, 2, 1)                # 0 / 0, a ratio below 1, a NaN mean
    per_block = Demodulator._snr_from_means(sig, noise)
    assert per_block.dtype == np.float32
    for b in range(64):
        with np.errstate(divide='ignore', invalid='ignore'):
            want = 20 * np.log10(sig[b] / noise[b] - 1)
        for got in (Demodulator._snr_from_means(sig[b], noise[b]), per_block[b]):
            assert type(got) is np.float32 and (got == want or (np.isnan(got) and np.isnan(want))), b
