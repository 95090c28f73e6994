"""Interference-peak clipping on the device (mfb_set_peak_clip, pycusdr_amd/csrc/clip_kernels.hpp) against the reference's
fixture G9 and the host's Demodulator._thresholdInput (reference DB:670-707): clipped samples bit for bit (through the
spectrum of the block), clippedPeakIPure exactly, single blocks, the chain from block to block and batches."""
import types

import numpy as np
import pytest

import clip_model as cm
from pycusdr_amd.demodulator.demodulator_base import Demodulator
from pycusdr_amd.mfbank import MFBank

pytestmark = pytest.mark.gpu

K = dict(k_offset=200, k_len=100, spsym_min=8)


def _bank(log2N, taps=32, seed=0):
    """A fixed-shift handle whose two filters have a short impulse response (segment path: batches run there)."""
    N = 1 << log2N
    rs = np.random.RandomState(seed)
    h = np.zeros((2, N), np.complex64)
    h[:, :taps] = rs.standard_normal((2, taps)) + 1j * rs.standard_normal((2, taps))
    bank = MFBank(log2N, 4, 2)
    bank.set_filters(np.conj(np.fft.fft(h, axis=1)).astype(np.complex64))
    bank.set_shifts([0, 1, 2, 3])
    return bank


def _host(x, scale):
    y = x.copy()
    s = types.SimpleNamespace(peakThresholdScale=scale, Nfft=len(x))
    Demodulator._thresholdInput(s, y)
    return y, np.asarray(s.clippedPeakIPure, dtype=np.int64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_block(clip_bank, plain_bank, x, scale, want_out, want_idx):
    N = len(x)
    clip_bank.set_peak_clip(scale, 0)
    clip_bank.input[:] = x
    r = clip_bank.receive_block(fixed_shift=0, **K)
    assert np.array_equal(r['clipped'], want_idx)
    got = clip_bank.get_spectrum(0, N)
    plain_bank.input[:] = want_out
    plain_bank.receive_block(fixed_shift=0, **K)
    assert np.array_equal(_bits(got), _bits(plain_bank.get_spectrum(0, N)))
    assert np.array_equal(_bits(clip_bank.input), _bits(x))       # the caller's samples stay as they were


def test_g9_cases_through_the_c_abi():
    g = np.load(__file__.rsplit('/', 1)[0] + '/golden/ref_goldens.npz')
    keys = sorted(k[:-4] for k in g.files if k.startswith('g9__') and k.endswith('__in'))
    assert len(keys) == 10
    a, b = _bank(12), _bank(12)
    try:
        for p in keys:
            scale = float(p.split('__s')[1])
            _check_block(a, b, g[p + '__in'].astype(np.complex64), scale, g[p + '__out'], g[p + '__clippedPeakIPure'])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('log2N', [15, 17, 20])
def test_random_bursts_equal_the_host_clip(log2N):
    a, b = _bank(log2N), _bank(log2N)
    rng = np.random.default_rng(log2N)
    try:
        for scale in (4.5, 40.5, 4.3):
            x = cm.bursty(rng, 1 << log2N)
            out, idx = _host(x, scale)
            assert len(idx)
            _check_block(a, b, x, scale, out, idx)
    finally:
        a.close()
        b.close()


def test_edge_cases():
    N = 1 << 15
    a, b = _bank(15), _bank(15)
    rng = np.random.default_rng(3)
    try:
        cases = [(np.zeros(N, np.complex64), 4.5)]
        x = cm.bursty(rng, N)
        x[1234] = np.nan
        cases.append((x, 4.5))
        cases.append((cm.bursty(rng, N, bursts=0), 1.0))                  # about half the block clips: the long list
        x = cm.bursty(rng, N, bursts=3)
        x[N - 7:] *= np.float32(500)                                      # a burst at the block's end
        cases.append((x, 4.5))
        for x, scale in cases:
            out, idx = _host(x, scale)
            _check_block(a, b, x, scale, out, idx)
        assert len(_host(cases[2][0], 1.0)[1]) > N // 4
    finally:
        a.close()
        b.close()


def _stream(rng, N, ov, nblocks):
    """A stream of nblocks blocks (stride N - ov) with bursts inside the last `ov` samples of blocks and just after block starts."""
    stride = N - ov
    n = nblocks * stride + ov
    at = []
    for k in range(1, nblocks + 1):
        at += [(k * stride + int(rng.integers(0, ov - 60)), 40), (k * stride + ov + int(rng.integers(0, 200)), 20)]
    return cm.bursty(rng, n, bursts=3 * nblocks, at=[(p, ln) for p, ln in at if p + ln < n])


def _host_chain(s, N, ov, nblocks, scale):
    stride = N - ov
    carry, outs, idxs = None, [], []
    for k in range(nblocks):
        x = s[k * stride:k * stride + N].copy()
        if carry is not None:
            x[:ov] = carry
        y, idx = _host(x, scale)
        carry = y[N - ov:].copy()
        outs.append(y)
        idxs.append(idx)
    return outs, idxs


@pytest.mark.parametrize('log2N,nblocks,B', [(15, 12, 1), (15, 12, 4), (17, 4, 1), (17, 4, 4)])
def test_chain_equals_the_host_loop(log2N, nblocks, B):
    """Block k's overlap is block k - 1's clipped tail (reference DP:293,337): one block per call and B per call, across calls."""
    N, ov, scale = 1 << log2N, 1 << 11, 4.5
    rng = np.random.default_rng(log2N * 100 + B)
    s = _stream(rng, N, ov, nblocks)
    outs, idxs = _host_chain(s, N, ov, nblocks, scale)
    assert sum(1 for k in range(nblocks - 1) if np.any(outs[k][N - ov:] != s[(k + 1) * (N - ov):(k + 1) * (N - ov) + ov])) >= 2
    a, b = _bank(log2N), _bank(log2N)
    stride = N - ov
    try:
        a.set_peak_clip(scale, ov)
        got = []
        if B == 1:
            for k in range(nblocks):
                a.input[:] = s[k * stride:k * stride + N]
                got.append(a.receive_block(fixed_shift=0, **K))
        else:
            wins = a.windows(B, stride)
            for k0 in range(0, nblocks, B):
                nb = min(B, nblocks - k0)
                w = wins[(k0 // B) % 2]
                w[:nb * stride + ov] = s[k0 * stride:(k0 + nb) * stride + ov]
                a.begin_blocks(0, nb, fixed_shift=0, source=('window', 'window2')[(k0 // B) % 2], **K)
                got += [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()} for d in a.end_blocks(0)]
        for k in range(nblocks):
            assert np.array_equal(got[k]['clipped'], idxs[k]), k
            b.input[:] = outs[k]
            want = b.receive_block(fixed_shift=0, **K)
            for key in ('cr', 'spSym', 'codeOffset', 'symbols', 'centres', 'magnitudes'):
                assert np.array_equal(np.asarray(got[k][key]), np.asarray(want[key])), (k, key)
        # restart: the next block's overlap is taken as given
        a.restart_peak_clip()
        x = s[:N].copy()
        x[:ov] = s[stride + 100:stride + 100 + ov]
        a.input[:] = x
        assert np.array_equal(a.receive_block(fixed_shift=0, **K)['clipped'], _host(x, scale)[1])
    finally:
        a.close()
        b.close()


def test_uploaded_input_is_refused_while_clipping():
    a = _bank(12)
    try:
        a.set_peak_clip(4.5, 0)
        a.upload(np.zeros(4096, np.complex64))
        with pytest.raises(ValueError):
            a.receive_block(fixed_shift=0, source='uploaded', **K)
        a.set_peak_clip(0)
        a.receive_block(fixed_shift=0, source='uploaded', **K)
    finally:
        a.close()


TIMING = ('timestamp', 'time_ms', 'rate_ksps', 'rate_ksps_avg', 'latency_ms')


def _eq(u, v):
    u, v = np.asarray(u), np.asarray(v)
    if u.dtype.kind in 'fc' and v.dtype.kind in 'fc':
        return u.shape == v.shape and np.array_equal(u, v, equal_nan=True)
    return np.array_equal(u, v)


def _stx_runners(bs, nblocks, seed):
    from pycusdr_amd import config as cfg, signals as sg
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.protocol import loadProtocol
    import copy
    N, ov = 1 << bs, 1 << 11
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, overlap=11, doppCarrierSteps=8)
    conf['GPU']['UHF']['peakThresholdScale'] = 4.5
    conf['Radios']['Rx']['UHF-H']['radioBackend'] = 'STX'
    dconf = copy.deepcopy(conf)
    dconf['GPU']['UHF'].setdefault('HIP', {})['device_clip'] = True
    p = loadProtocol('bench_GMSK')(conf=conf)
    host, dev = DemodulatorRunner(conf, p, 'UHF-H'), DemodulatorRunner(dconf, p, 'UHF-H')
    assert dev.demod._device_clip and not host.demod._device_clip
    sig = sg.s1_stream(nblocks, N, ov, 'GMSK', snr_db=12.0, seed=seed)
    rng = np.random.default_rng(seed)
    stride = N - ov
    for k in range(1, nblocks):       # bursts inside the last `ov` samples of blocks and just after block starts
        for p0, ln in ((k * stride + int(rng.integers(0, ov - 60)), 30), (k * stride + ov + int(rng.integers(0, 64)), 12)):
            sig[p0:p0 + ln] *= np.float32(rng.uniform(50, 400))
    return conf, p, host, dev, sig[ov:]


@pytest.mark.parametrize('bs,nblocks,B', [(15, 12, 1), (15, 12, 4), (17, 4, 1), (17, 4, 4)])
def test_stx_stream_with_device_clip_equals_host_clip(bs, nblocks, B):
    from pycusdr_amd.decoder import Decoder
    conf, p, host, dev, sig = _stx_runners(bs, nblocks, seed=bs + B)
    batches = []
    inner = dev.demod.beginBlocks
    dev.demod.beginBlocks = lambda slot, nb, **kw: (batches.append(nb), inner(slot, nb, **kw))[1]
    try:
        chunks = lambda: (sig[i:i + 20000] for i in range(0, len(sig), 20000))
        ra, pa = host.run_stream(chunks(), decoder=Decoder(conf, p), blocks_per_call=B)
        rb, pb = dev.run_stream(chunks(), decoder=Decoder(conf, p), blocks_per_call=B)
        assert len(ra) == len(rb) == nblocks
        if B > 1:       # the batched loop ran, with batches of B blocks (and the shorter last one)
            assert sum(batches) == nblocks and max(batches) == B and len(batches) == -(-nblocks // B), batches
        else:
            assert not batches
        assert sum(1 for d in ra if (np.asarray(d['trust']) == 254).any()) >= 2       # clipped peaks were tagged
        for x, y in zip(ra, rb):
            keys = set(x) - set(TIMING)
            assert keys == set(y) - set(TIMING)
            for k in keys:
                assert _eq(x[k], y[k]), (x['count'], k)
        assert len(pa) == len(pb) and all(np.array_equal(u.bits, v.bits) for u, v in zip(pa, pb))
        assert np.array_equal(host.demod.clippedPeakIPure, dev.demod.clippedPeakIPure)
        assert np.array_equal(host.demod.clippedPeakI, dev.demod.clippedPeakI)
    finally:
        host.close()
        dev.close()


def test_stx_feed_resident_with_device_clip_equals_feed():
    import torch
    conf, p, host, dev, sig = _stx_runners(15, 2, seed=9)
    try:
        N, ov = host.blockSize, host.overlap
        block = np.concatenate((np.zeros(ov, np.complex64), sig[:N - ov]))
        want = host.feed_host(host.feed_device(sig[:N - ov].copy()))
        t = torch.from_numpy(block.view(np.float32).copy()).cuda()
        got = dev.feed_host(dev.feed_resident(t.data_ptr()))
        torch.cuda.synchronize()
        for k in set(want) - set(TIMING):
            assert _eq(want[k], got[k]), k
        assert np.array_equal(host.demod.clippedPeakIPure, dev.demod.clippedPeakIPure)
    finally:
        host.close()
        dev.close()


def test_host_block_after_device_blocks_carries_the_clipped_tail():
    """A block clipped on the host after device-clipped blocks takes their clipped tail as its overlap (reference DP:293,337)."""
    conf, p, host, dev, sig = _stx_runners(15, 4, seed=21)
    try:
        sps = host.samplesPerSlice
        new = [sig[k * sps:(k + 1) * sps].copy() for k in range(4)]
        want = [host.feed(x.copy()) for x in new]
        got = []
        for x in new[:3]:
            dev.feed_device_begin(x.copy())
            got.append(dev.feed_host(dev.feed_device_end()))
        got.append(dev.feed(new[3].copy()))                  # the host path: the device clip is switched off for it
        for w, g in zip(want, got):
            for k in set(w) - set(TIMING):
                assert _eq(w[k], g[k]), (w['count'], k)
        assert np.array_equal(host.demod.clippedPeakIPure, dev.demod.clippedPeakIPure)
    finally:
        host.close()
        dev.close()


def test_a_pending_flight_keeps_its_clips_when_a_larger_batch_begins():
    N, ov, scale = 1 << 15, 1 << 11, 4.5
    stride = N - ov
    rng = np.random.default_rng(31)
    a = _bank(15)
    try:
        a.set_peak_clip(scale, 0)
        x = cm.bursty(rng, N)
        a.input[:] = x
        a.begin_block(0, fixed_shift=0, **K)                  # pending in slot 0 (one block of clip buffers)
        s = _stream(rng, N, ov, 4)
        w = a.windows(4, stride)[0]
        w[:] = s[:4 * stride + ov]
        a.begin_blocks(1, 4, fixed_shift=0, source='window', **K)     # a larger batch in slot 1
        r0 = a.end_block(0)
        r1 = a.end_blocks(1)
        assert np.array_equal(r0['clipped'], _host(x, scale)[1])
        for k in range(4):
            assert np.array_equal(r1[k]['clipped'], _host(s[k * stride:k * stride + N], scale)[1]), k
        assert np.array_equal(a.get_block_clips(0), _host(x, scale)[1])     # slot 0's list survives slot 1's batch
    finally:
        a.close()


def test_rate_stage_on_an_all_nan_window_stays_inside_it():
    """A block with a NaN sample makes the whole rate window NaN: the argmax has no ordered value and takes the window's first
    bin (numpy's argmax returns the first NaN) instead of reading outside the spectrum."""
    a = _bank(15)
    try:
        x = cm.bursty(np.random.default_rng(4), 1 << 15)
        x[77] = np.nan
        a.input[:] = x
        r = a.receive_block(fixed_shift=0, **K)
        assert r['cr'][0] == np.float32(K['k_offset'])
    finally:
        a.close()
