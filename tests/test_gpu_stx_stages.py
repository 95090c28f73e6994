"""S-band (STX) batches finished on the device: with the device clip, mfb_receive_blocks_* at a fixed shift run the bit lookup, the
block-overlap alignment, the decoder's searches and the clipped-peak tags (k_stream_tag, reference DB:830-837) -- against the
one-block loop with the host clip and the same batches with "stream_stages": false, bit for bit; and the tag through the plain
C ABI against the numpy model of tests/stx_tag_model.py."""
import ctypes as C

import numpy as np
import pytest

import stx_tag_model as tm

pytestmark = pytest.mark.gpu

TIMING = ('timestamp', 'time_ms', 'rate_ksps', 'rate_ksps_avg', 'latency_ms')
OV = 1 << 11
MODS = {'bench_GMSK': 'GMSK', 'bench_BPSK': 'BPSK'}


def _eq(u, v):
    u, v = np.asarray(u), np.asarray(v)
    if u.dtype.kind in 'fc' and v.dtype.kind in 'fc':
        return u.shape == v.shape and np.array_equal(u, v, equal_nan=True)
    return u.shape == v.shape and np.array_equal(u, v)


def _conf(pname, bs, device_clip, **hip):
    from pycusdr_amd import config as cfg
    conf = cfg.bench_config(pname, blockSize=bs, overlap=11, doppCarrierSteps=8)
    conf['GPU']['UHF']['peakThresholdScale'] = 4.5
    conf['Radios']['Rx']['UHF-H']['radioBackend'] = 'STX'
    h = conf['GPU']['UHF'].setdefault('HIP', {})
    h['device_clip'] = device_clip
    h.update(hip)
    return conf


def _run(pname, bs, sig, device_clip, B=1, watch=False, **hip):
    """run_stream of `sig` (chunks of 20000 samples) with a Decoder: (results, packets, the demodulator's end state, the
    per-block (spSym, clip indices, kept centres) of the host stage when `watch`).  The end state lists the blocks whose
    A12 / A13 the device ran ('device_blocks')."""
    from pycusdr_amd.decoder import Decoder
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.protocol import loadProtocol
    conf = _conf(pname, bs, device_clip, **hip)
    p = loadProtocol(pname)(conf=conf)
    r = DemodulatorRunner(conf, p, 'UHF-H')
    seen, order, dev_blocks = [], [], []
    try:
        assert r.demod._device_clip == device_clip
        d = r.demod
        inner_h, inner_c = d.demodulateHost, d.checkSymbolOverlap

        def check(*a):
            out = inner_c(*a)
            if watch:
                seen[-1].append(np.asarray(out[0]).copy())
            return out

        def host(rec, prev_tail=None):
            k = len(order)
            order.append(k)
            if watch:
                seen.append([float(rec['spSym']), np.asarray(rec['clipped']).copy()])
            before = getattr(d, 'stage_blocks', 0)
            out = inner_h(rec, prev_tail=prev_tail)
            if getattr(d, 'stage_blocks', 0) > before:
                dev_blocks.append(k)
            return out
        d.demodulateHost, d.checkSymbolOverlap = host, check
        dec = Decoder(conf, p)
        res, pk = r.run_stream((sig[i:i + 20000] for i in range(0, len(sig), 20000)), decoder=dec, blocks_per_call=B)
        d = r.demod
        state = {'poswinP': np.asarray(d.poswinP).copy(), 'posSymEnd': np.asarray(d.posSymEnd).copy(),
                 'clippedPeakIPure': np.asarray(d.clippedPeakIPure).copy(), 'clippedPeakI': np.asarray(d.clippedPeakI).copy(),
                 'bitsOverlapBuf': np.asarray(dec.bitsOverlapBuf).copy(), 'stage_blocks': int(getattr(d, 'stage_blocks', 0)),
                 'device_blocks': dev_blocks}
    finally:
        r.close()
    return res, pk, state, seen


def _same_runs(a, b, nblocks):
    ra, pa, sa, _ = a
    rb, pb, sb, _ = b
    assert len(ra) == len(rb) == nblocks
    for x, y in zip(ra, rb):
        keys = set(x) - set(TIMING)
        assert keys == set(y) - set(TIMING)
        for k in keys:
            assert _eq(x[k], y[k]), (x['count'], k)
    assert len(pa) == len(pb) and all(np.array_equal(u.bits, v.bits) for u, v in zip(pa, pb))
    for k in ('poswinP', 'posSymEnd', 'bitsOverlapBuf', 'clippedPeakIPure', 'clippedPeakI'):
        assert _eq(sa[k], sb[k]), k


def _three_ways(pname, bs, sig, nblocks, Bs, watch=False, **hip):
    ref = _run(pname, bs, sig, False, 1, watch=watch)
    for B in Bs:
        host_st = _run(pname, bs, sig, True, B, stream_stages=False, **hip)
        dev_st = _run(pname, bs, sig, True, B, **hip)
        _same_runs(ref, host_st, nblocks)
        _same_runs(ref, dev_st, nblocks)
        yield B, ref, host_st, dev_st


@pytest.mark.parametrize('pname', ['bench_GMSK', 'bench_BPSK'])
@pytest.mark.parametrize('bs,nblocks', [(15, 40), (17, 36)])
def test_burst_stream_equals_the_one_block_host_loop(pname, bs, nblocks):
    N = 1 << bs
    full = tm.make_stream(MODS[pname], N, OV, nblocks, tm.burst_bursts(N, OV, nblocks, seed=bs), seed=bs)
    checked = False
    for B, ref, host_st, dev_st in _three_ways(pname, bs, full[OV:], nblocks, (4, 16), watch=True):
        if not checked:
            # the input: clipped peaks are tagged in a quarter of the blocks, and kept centres sit exactly 2 s and 2 s + 1
            # from a clip index (the tag's last marked sample and the first unmarked one)
            ra, seen = ref[0], ref[3]
            assert sum(1 for d in ra if (np.asarray(d['trust']) == 254).any()) * 4 >= nblocks
            at, past = 0, 0
            for sp, P, cw in seen:
                s = int(np.ceil(sp))
                if len(P) and len(cw):
                    d = np.abs(cw.astype(np.int64)[:, None] - P[None, :])
                    at += int((d == 2 * s).any())
                    past += int((d == 2 * s + 1).any())
            assert len(seen) == nblocks and at >= 1 and past >= 1, (at, past)
            checked = True
        assert host_st[2]['stage_blocks'] == 0
        assert dev_st[2]['stage_blocks'] >= nblocks - 2 * B - 1, (B, dev_st[2]['stage_blocks'])


@pytest.mark.parametrize('pname', ['bench_GMSK', 'bench_BPSK'])
@pytest.mark.parametrize('bs', [15, 17])
def test_edge_stream_equals_the_one_block_host_loop(pname, bs):
    N, nblocks = 1 << bs, tm.EDGE_BLOCKS
    full = tm.make_stream(MODS[pname], N, OV, nblocks, tm.edge_bursts(N, OV, nblocks), seed=5)
    for B, ref, host_st, dev_st in _three_ways(pname, bs, full[OV:], nblocks, (4, 16)):
        assert host_st[2]['stage_blocks'] == 0
        assert dev_st[2]['stage_blocks'] >= nblocks - 2 * B - 1, dev_st[2]['stage_blocks']


def test_c_abi_fixed_shift_batch_runs_the_stages_and_the_tag():
    """mfb_set_stream_stages + mfb_set_peak_clip, then an MFB_BLOCK_FIXED_SHIFT batch through mfb_receive_blocks_begin /
    _end_record: layout.stream_stages == 1, the kept trust bytes are the model's tag of the record's own kept window, full
    centres and mfb_get_block_clips, and the kept bits / centres are the host's extractBits / checkSymbolOverlap."""
    from pycusdr_amd import _lib
    from pycusdr_amd.demodulator import STX
    from pycusdr_amd.demodulator.demodulator_base import TRUSTTYPE, Operations
    from pycusdr_amd.mfbank import BLOCK_SCALARS
    from pycusdr_amd.protocol import loadProtocol
    bs, nb = 15, 6
    N = 1 << bs
    stride = N - OV
    conf = _conf('bench_GMSK', bs, True)
    p = loadProtocol('bench_GMSK')(conf=conf)
    d, h = STX.Demodulator(conf, p, 'UHF-H'), STX.Demodulator(conf, p, 'UHF-H')
    try:
        lib, bank = _lib.load(), d.bank
        assert d.enableStreamStages() and d.seedStreamStages()
        d._armDeviceClip(True)
        full = tm.make_stream('GMSK', N, OV, nb, tm.burst_bursts(N, OV, nb, seed=3), seed=3)
        full[:OV] = full[OV:2 * OV]              # (no stretch of zeros at the start: every block is a regular one)
        w = d.blockWindows(nb)[0]
        w[:nb * stride + OV] = full[:nb * stride + OV]
        P = bank._block_params(d.codeRateAndPhaseOffsetHigh, d.codeRateAndPhaseOffsetLow - d.codeRateAndPhaseOffsetHigh, d.spsymMin,
                               Operations.CENTRES_ABS.value, 5, int(d.doppOffsetIdx), 'window', None)
        assert lib.mfb_receive_blocks_begin(bank._h, C.byref(P), nb, 0) == 0
        lay = _lib.RecordLayout()
        buf = np.empty(64 << 20, np.uint8)
        assert lib.mfb_receive_blocks_end_record(bank._h, 0, buf.ctypes.data, buf.size, C.byref(lay)) == 0
        assert lay.stream_stages == 1 and lay.mode == 1 and lay.nblocks == nb
        rec = buf[:nb * lay.record_bytes].reshape(nb, lay.record_bytes)
        tagged = 0
        for b in range(nb):
            sc = rec[b, :BLOCK_SCALARS.itemsize].copy().view(BLOCK_SCALARS)[0]
            n = int(sc['count'])
            sym = rec[b, lay.off_sym:lay.off_sym + 4 * n].view(np.int32)
            cen = rec[b, lay.off_cen:lay.off_cen + 4 * n].view(np.int32)
            trust_all = rec[b, lay.off_mag:lay.off_mag + 4 * n].view(TRUSTTYPE)[:n]
            cnt = C.c_int32(0)
            idx = np.empty(N, np.int32)
            assert lib.mfb_get_block_clips(bank._h, 0, b, idx.ctypes.data, idx.size, C.byref(cnt)) == 0
            clips = idx[:cnt.value].astype(np.int64)
            assert sc['a13_status'] != 0 and sc['clip_tag'] == 1 and sc['clip_count'] == len(clips), (b, sc['a13_status'])
            start, nw = int(sc['a13_start']), int(sc['a13_nwin'])
            bits = rec[b, lay.off_bits:lay.off_bits + nw]
            cen8 = rec[b, lay.off_centres_u8:lay.off_centres_u8 + nw]
            trust = rec[b, lay.off_trust:lay.off_trust + nw]
            # the host's A12 / A13 on the record's own symbols, in order from the same (empty) state
            dataBits, noErr = h.extractBits(cen, sym)
            cw, bw, tw, _ = h.checkSymbolOverlap(len(noErr), cen, sym, dataBits, trust_all.copy())
            assert np.array_equal(bits, bw.astype(np.uint8)) and np.array_equal(cen8, cw.astype(np.uint8)), b
            assert np.array_equal(cw, cen[start:start + nw]), b
            # the tag: the model on the record's kept window and full centres, and the literal host loop
            want = tm.tag(trust_all[start:start + nw], cen[start:start + nw], clips, float(sc['spSym']), N)
            assert np.array_equal(trust, want), b
            assert np.array_equal(trust, tm.host_tag(tw, cw, clips, float(sc['spSym']), N)), b
            tagged += int((trust == 254).any())
        assert tagged >= 2
    finally:
        d.close()
        h.close()


@pytest.mark.parametrize('case', ['b70', 'batch_overlap', 'irregular'])
def test_fallbacks_equal_the_one_block_host_loop(case):
    pname, bs = 'bench_GMSK', 15
    N = 1 << bs
    nblocks, B, hip = {'b70': (73, 70, {}), 'batch_overlap': (20, 4, {'batch_overlap': True}), 'irregular': (28, 4, {})}[case]
    full = tm.make_stream('GMSK', N, OV, nblocks, tm.burst_bursts(N, OV, nblocks, seed=nblocks), seed=nblocks)
    zeroed = 13
    if case == 'irregular':
        # noiseless zero padding: one block of nothing (symbol index -1 -- outside the LUT) goes to the host code
        full[zeroed * (N - OV):zeroed * (N - OV) + N] = 0
    for _, ref, host_st, dev_st in _three_ways(pname, bs, full[OV:], nblocks, (B,), **hip):
        assert host_st[2]['stage_blocks'] == 0
        n = dev_st[2]['stage_blocks']
        if case == 'b70':
            assert n <= nblocks - B, n                      # only the short last batch could run its stages on the device
        elif case == 'irregular':
            # the irregular blocks (zeroed - 1 ... zeroed + 1) went to the host; the device chain ran in front of them, re-seeded
            # and resumed behind them
            dev = dev_st[2]['device_blocks']
            assert not set(dev) & {zeroed - 1, zeroed, zeroed + 1}, dev
            assert any(k < zeroed - 1 for k in dev) and any(k > zeroed + 1 for k in dev), dev
        else:
            assert n >= nblocks - 2 * B - 1, n
