"""One process of tests/test_gpu_flight_paths.py: the same input submitted again and again with the same parameters, so that
the flight goes out as plain launches (first call), is captured into a graph and launched (second), and replays it (third,
fourth); everything the library hands back is kept, raw, for the test to compare.
usage: flight_child.py block|batch overlap(0|1) out.npz

block: one 2^15-sample block from the page-locked input buffer, four calls.
batch: three blocks from a page-locked window with the stream stages on and band capacity 0, eight calls -- the batch's graphs
are kept per carry parity, which every batch with stages flips, so each parity sees four -- the carry seeded afresh before
each; then the debug seam of the stream stages on the same handle for the same symbol count."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from pycusdr_amd import _lib, config as cfg, signals as sg      # noqa: E402
from pycusdr_amd.decoder import Decoder                        # noqa: E402
from pycusdr_amd.demodulator import UHF                        # noqa: E402
from pycusdr_amd.mfbank import _ptr                            # noqa: E402
from pycusdr_amd.protocol import loadProtocol                  # noqa: E402

kind, overlap, out = sys.argv[1], bool(int(sys.argv[2])), sys.argv[3]
bs, ov, B = 15, 1 << 10, 3
N = 1 << bs
step = N - ov
conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
proto = loadProtocol('bench_GMSK')(conf=conf)
demod = UHF.Demodulator(conf, proto, 'UHF-H')
bank, lib = demod.bank, demod.bank._lib
sig = sg.s1_stream(B + 1, N, ov, 'GMSK', snr_db=20.0, seed=1)
LAY_FIELDS = [k for k, _ in _lib.RecordLayout._fields_]
res = {}

if kind == 'block':
    bank.set_batch_overlap(overlap)
    demod.get_signalBufferHostPointer()[:] = sig[step:step + N]          # the second block: inside the packet
    cap, bcap = N // 2, bank.BAND_CAPACITY
    results, syms, cens, mags, bands = [], [], [], [], []
    for call in range(4):
        demod.beginBlock(0, source='pinned')
        R = _lib.BlockResult()
        sym, cen, mag = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        band = np.zeros((2, bcap), np.complex64)
        _lib.check(lib.mfb_receive_block_end(bank._h, 0, C.byref(R), _ptr(sym), _ptr(cen), _ptr(mag), _ptr(band)), 'mfb_receive_block_end')
        bank._flying.discard(0)
        results.append(np.frombuffer(bytes(R), np.uint8))
        syms.append(sym)
        cens.append(cen)
        mags.append(mag)
        bands.append(band)
    res = dict(result=np.array(results), count=np.int64(R.count), band_len=np.array(R.band_len[:], np.int64), sym=np.array(syms),
               cen=np.array(cens), mag=np.array(mags), bands=np.array(bands))
else:
    bank.BAND_CAPACITY = 0           # as the debug seam reports it
    bank.set_batch_overlap(overlap)
    demod.blockWindows(B)[0][:] = sig[:B * step + ov]
    assert demod.enableStreamStages(Decoder(conf, proto))
    recs, lays = [], []
    for call in range(8):
        assert demod.seedStreamStages()
        demod.beginBlocks(0, B, source='window')
        lay = _lib.RecordLayout()
        buf = np.zeros(1 << 20, np.uint8)
        _lib.check(lib.mfb_receive_blocks_end_record(bank._h, 0, _ptr(buf), buf.size, C.byref(lay)), 'mfb_receive_blocks_end_record')
        bank._flying.discard(0)
        recs.append(buf[:lay.nblocks * lay.record_bytes].copy())
        lays.append([int(getattr(lay, k)) for k in LAY_FIELDS])
    n = int(lay.symbols)
    dbg = _lib.RecordLayout()
    buf = np.zeros(1 << 20, np.uint8)
    zi, zf = np.zeros((B, n), np.int32), np.zeros((B, n), np.float32)
    _lib.check(lib.mfb_debug_stream_stages(bank._h, B, n, _ptr(np.zeros(B, np.int32)), _ptr(zi), _ptr(zi), _ptr(zf), _ptr(buf), buf.size,
                                           C.byref(dbg)), 'mfb_debug_stream_stages')
    res = dict(records=np.array(recs), layouts=np.array(lays, np.int64), debug_layout=np.array([int(getattr(dbg, k)) for k in LAY_FIELDS], np.int64))
np.savez(out, **res)
demod.close()
