"""computeSNR's two window means on the device (mfb_set_device_snr, csrc/snr_kernels.hpp; reference demodulator_base.py:635-667):
the kernel on injected spectra and windows against numpy, the pick -> pieces -> means chain for every neighbouring pair of a sparse
bin table against ``Demodulator.computeSNR``, and the mode through every public call path -- one block, batches (the blocks whose
windows are longer than what travels with a batch: NaN without the mode, the one-block loop's SNR with it), batches on two streams
-- bit for bit; with the mode off not a byte of a record changes."""
import ctypes as C
import warnings

import numpy as np
import pytest

from pycusdr_amd import _lib, config as cfg, mfbank, signals as sg
from pycusdr_amd.demodulator import UHF
from pycusdr_amd.demodulator.demodulator_base import Demodulator
from pycusdr_amd.protocol import loadProtocol

import snr_model as sm
from snr_model import LENGTHS, PAIRS

pytestmark = pytest.mark.gpu


def _host_mean(X, w):
    (s0, n0), (s1, n1) = w
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)            # "Mean of empty slice"
        return np.float32(np.mean(np.abs(np.concatenate((X[s0:s0 + n0], X[s1:s1 + n1])))))


def _windows(N):
    """The lengths of the CPU test at starts 0, 1, N - len and across N / 2; wrap windows (piece 0 reaching N, piece 1 from 0);
    empty windows; the whole spectrum."""
    out = []
    for i, n in enumerate(LENGTHS):
        starts = (0, 1, N - n, N // 2 - n // 2)
        for s in (starts if n > 300 or n in (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257) else (starts[i % 4],)):
            if 0 <= s and s + n <= N:
                out.append(((s, n), (0, 0)))
    out += [((N - a, a), (0, b)) for a, b in PAIRS]
    out += [((5, 0), (7, 0)), ((N, 0), (N, 0)), ((0, N), (0, 0)), ((N // 2, N // 2), (0, N // 2)), ((3, N - 3), (0, 3))]
    return out


def test_seam_against_numpy():
    N = 1 << 15
    X = sm.spread(np.random.default_rng(5), N)
    wins = _windows(N)
    want = np.array([_host_mean(X, w) for w in wins])
    # the inputs tell numpy's order from a plain sum for most windows above 128 elements (one shared spectrum: not for every one)
    long_ = [w for w in wins if w[0][1] + w[1][1] > 128]
    told = sum(sm.left_to_right(m) != np.add.reduce(m)
               for m in (np.abs(np.concatenate((X[a:a + n], X[b:b + k]))) for (a, n), (b, k) in long_))
    assert len(wins) >= 80 and told > 0.6 * len(long_)
    got = mfbank.debug_band_means(X, np.array(wins, np.int32))
    bad = [(w, g, r) for w, g, r in zip(wins, got, want) if not sm.same_bits(g, r)]
    assert not bad, bad[:5]
    assert np.isnan(got[[i for i, w in enumerate(wins) if w[0][1] + w[1][1] == 0]]).all()
    # the same call on a second, identical spectrum: the same bits
    again = mfbank.debug_band_means(X.copy(), np.array(wins, np.int32))
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # an inf and a NaN element (either part), inside short, leaf-sized, chunk-sized and two-piece windows
    for bad_value in (np.inf, np.nan):
        for part in ('real', 'imag'):
            Y = X.copy()
            getattr(Y, part)[[3, 1000, N - 2]] = bad_value
            ws = [((0, 5), (0, 0)), ((0, 131), (0, 0)), ((900, 300), (0, 0)), ((0, 8199), (0, 0)), ((N - 100, 100), (0, 2)),
                  ((N - 1, 1), (0, 20)), ((4, 900), (0, 0)), ((0, N), (0, 0))]
            g = mfbank.debug_band_means(Y, np.array(ws, np.int32))
            r = np.array([_host_mean(Y, w) for w in ws])
            assert sm.same_bits(g, r), (bad_value, part, g, r)
            assert np.isfinite(g[6]) and not np.isfinite(g[[0, 1, 3, 4, 5, 7]]).any()
    with pytest.raises(ValueError):
        mfbank.debug_band_means(X, np.array([((N - 3, 4), (0, 0))], np.int32))


def _stream(nb, N, ov, seed):
    """``nb`` blocks of the noisy packet stream from inside the packet (the stream begins with 10000 samples of padding: noise alone)."""
    skip = -(-12000 // (N - ov))
    return sg.s1_stream(nb + skip, N, ov, 'GMSK', snr_db=9.0, seed=seed)[skip * (N - ov):]


def _demod(bs, D, hip=None, **kw):
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=D, **kw)
    if hip:
        conf['GPU']['UHF']['HIP'] = dict(hip)
    return UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H')


def test_pick_to_pieces_to_means_for_every_pair():
    """A sparse shift table at 2^13 whose neighbouring pairs give windows below 256, between 256 and 1024 and above 1024 elements,
    one pair wrapping around 0 Hz; a pick on and between every pair."""
    bs, ov = 13, 1 << 10
    N = 1 << bs
    d = _demod(bs, 8)
    try:
        table = np.array([100, 200, 600, 1900, 2100, 5000, 8000, 150], np.int32)
        d.doppCyperSymNorm = table
        d.bank.set_shifts(table)
        cap, longest = d._snr_band_capacity(5)
        assert longest == 3010 and cap == 4096
        d.bank.upload(_stream(1, N, ov, 2)[:N])
        X = d.bank.get_spectrum()
        picks = [(i, 1.0) for i in range(8)] + [(i + f, 1.0) for i in range(7) for f in (0.5, 0.03125)]
        rs = d.bank.debug_block_scalars(np.array(picks, np.float32), np.tile(np.float32([N / 16, 0.1, 1.0]), (len(picks), 1)), d.spsymMin)
        pieces = np.array([r['band_pieces'] for r in rs], np.int32)
        means = mfbank.debug_band_means(X, pieces.reshape(-1, 2, 2)).reshape(-1, 2)
        lens = set()
        for r, m in zip(rs, means):
            assert r['pick_valid']
            got = Demodulator._snr_from_means(m[0], m[1])
            want = d.computeSNR(r['low'], r['high'], 5)          # nothing in flight: through the spectrum slices
            assert sm.same_bits(got, want), (r['low'], r['high'], got, want)
            # (a ratio below 1 makes both NaN: the means themselves, too)
            assert sm.same_bits(m, [_host_mean(X, tuple(map(tuple, w))) for w in r['band_pieces']])
            lens.update(r['band_len'])
        assert min(lens) < 256 and any(256 <= x <= 1024 for x in lens) and max(lens) > 1024
    finally:
        d.close()


def _same(a, b):
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


def test_one_block_through_the_public_path():
    bs, ov = 13, 1 << 10
    N = 1 << bs
    sig = _stream(1, N, ov, 4)[:N]
    on, off = _demod(bs, 16, {'device_snr': True}), _demod(bs, 16)
    try:
        a, b = on.uploadAndFindCarrier(sig), off.uploadAndFindCarrier(sig)
        assert off._pending['pick_valid'] and np.isfinite(b[3]) and b[3] != 0 and type(a[3]) is type(b[3])
        assert _same([a[0], a[1], a[3]], [b[0], b[1], b[3]]) and _same(a[2], b[2]), (a, b)
        (ms, mn), lens = on.bank.block_snr(0, 0)
        assert lens == tuple(len(w) for w in off._pending['bands']) == on._pending['band_len']
        assert sm.same_bits([ms, mn], [np.mean(np.abs(w)) for w in off._pending['bands']])
        for k in ('symbols', 'centres', 'magnitudes'):
            assert _same(on._pending[k], off._pending[k]), k
    finally:
        on.close()
        off.close()


def _batch(d, sig, nb, N, ov, slot=0):
    step = N - ov
    w = d.blockWindows(nb)[slot]
    w[:nb * step + ov] = sig[:nb * step + ov]
    d.beginBlocks(slot, nb, source=('window', 'window2')[slot])
    return d.endBlocks(slot)


def _check_block(tag, got, want, snr=True):
    (ea, ra), (eb, rb) = got, want
    assert _same([ea[0], ea[1]] + ([ea[3]] if snr else []), [eb[0], eb[1]] + ([eb[3]] if snr else [])), (tag, ea, eb)
    assert ra['spSym'] == rb['spSym'], tag
    for k in ('symbols', 'centres', 'trust'):
        assert _same(ra[k], rb[k]), (tag, k)


def test_the_nan_hole():
    """Three bins 9335 spectrum bins apart at N = 2^15: every pick lies between two of them, its windows are 9345 elements long.
    The Demodulator plans room for windows of up to 2^16 elements, so at this block length it would deliver them; the test gives the
    handles without the key the room a batch has where the plan is capped (N >= 2^17) -- less than the window -- and keeps the block
    small."""
    bs, ov, nb = 15, 1 << 10, 3
    N = 1 << bs
    step = N - ov
    geo = dict(rangeRateMax=30000)
    sig = sg.s1_stream(nb, N, ov, 'GMSK', snr_db=9.0, seed=11)
    bat_off, bat_on, one = _demod(bs, 3, **geo), _demod(bs, 3, {'device_snr': True}, **geo), _demod(bs, 3, **geo)
    try:
        assert bat_off._snr_band_capacity(5)[1] > 8192
        bat_off.bank.BAND_CAPACITY = one.bank.BAND_CAPACITY = 4096
        holes = _batch(bat_off, sig, nb, N, ov)
        assert any(np.isnan(est[3]) for est, _ in holes)              # what the mode is for
        got = _batch(bat_on, sig, nb, N, ov)
        for b in range(nb):
            raw = one.get_signalBufferHostPointer()
            raw[:] = sig[b * step: b * step + N]
            est = one.uploadAndFindCarrier(raw)                       # the windows do not fit: fetched afterwards (nothing in flight)
            assert one._pending['bands'] is None and np.isfinite(est[3])
            assert not np.isnan(got[b][0][3]) and sm.same_bits(got[b][0][3], est[3]), (b, got[b][0], est)
            _check_block(b, got[b], (est, one.demodulateDevice()))
            _check_block(b, got[b], holes[b], snr=False)
            assert bat_on.bank.block_snr(0, b)[1] == (9345, 9345)
    finally:
        for d in (bat_off, bat_on, one):
            d.close()


def _raw_record(bank, slot):
    """The batch begun in ``slot`` as mfb_receive_blocks_end_record hands it out: its bytes."""
    lay = _lib.RecordLayout()
    buf = np.empty(1 << 22, np.uint8)
    _lib.check(bank._lib.mfb_receive_blocks_end_record(bank._h, slot, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(lay)),
               'mfb_receive_blocks_end_record')
    bank._flying.discard(slot)
    return buf[:lay.nblocks * lay.record_bytes].copy()


def test_off_means_off():
    bs, ov, nb = 13, 1 << 10, 2
    N = 1 << bs
    sig = _stream(nb, N, ov, 6)
    d = _demod(bs, 16)
    try:
        def record():
            w = d.blockWindows(nb)[0]
            w[:] = sig
            d.beginBlocks(0, nb)
            return _raw_record(d.bank, 0)
        first, before = record(), record()
        d.bank.set_device_snr(True)
        d.bank.set_device_snr(False)
        after = record()
        assert np.array_equal(first, before) and np.array_equal(before, after)
        with pytest.raises(RuntimeError):
            d.bank.block_snr(0, 0)
    finally:
        d.close()


def test_batch_overlap_gives_the_same_snr():
    bs, ov, nb = 13, 1 << 10, 4
    N = 1 << bs
    sig = _stream(nb, N, ov, 8)
    d = _demod(bs, 16, {'device_snr': True})
    try:
        want = _batch(d, sig, nb, N, ov)
        assert all(np.isfinite(est[3]) and est[3] != 0 for est, _ in want)
        d.bank.set_batch_overlap(True)
        for turn in range(3):                   # plain launches, the recording, a replay -- alternating slots
            got = _batch(d, sig, nb, N, ov, slot=turn & 1)
            for b in range(nb):
                _check_block((turn, b), got[b], want[b])
        d.bank.set_batch_overlap(False)
        for b, g in enumerate(_batch(d, sig, nb, N, ov)):
            _check_block(('off again', b), g, want[b])
    finally:
        d.close()


def test_switching_with_a_flight_begun_is_refused():
    bs, ov, nb = 13, 1 << 10, 2
    N = 1 << bs
    sig = _stream(nb, N, ov, 9)
    d = _demod(bs, 16, {'device_snr': True})
    try:
        want = _batch(d, sig, nb, N, ov)
        assert all(np.isfinite(est[3]) and est[3] != 0 for est, _ in want)
        w = d.blockWindows(nb)[0]
        w[:] = sig
        d.beginBlocks(0, nb)
        for on in (False, True):
            rc = d.bank._lib.mfb_set_device_snr(d.bank._h, int(on))
            assert rc == _lib.MFB_ERR_STATE
            with pytest.raises(RuntimeError):
                _lib.check(rc, 'mfb_set_device_snr')
        got = d.endBlocks(0)
        for b in range(nb):
            _check_block(b, got[b], want[b])
    finally:
        d.close()
