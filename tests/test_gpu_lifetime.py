"""Lifetime of what a handle owns (csrc/hip_owned.hpp): a handle whose buffers have all been regrown computes what a fresh handle
computes, and create / use / close cycles give their memory back.

A. Every grow-only reserve of the bank (csrc/bank_ctx.hpp and the bank's parts beside it) and the sync finder's are driven through
   their regrow branch -- the old buffer exists and is too small -- and the result is compared with a handle that was sized for the
   work from the start.  Which call reaches which branch:
     batch_reserve (work buffers, d_Z, the records, d_Z2), clip_reserve (flight buffers, workspace), staging_reserve:
         a batch of 1, of 3, of 8.  The library sizes these for the WINDOWS' capacity, not for the batch (one set of buffers serves
         batches of 1 ... B), so batches of growing size on the same windows regrow nothing: the windows are remade for 1, 3 and 8
         blocks, which also takes window_buffer's own remake branch twice (and frees the integer staging d_raw[2..3] with them).
     clip_reserve's tail: set_peak_clip with a larger overlap.
     blkout_reserve, staging_reserve (single block): a larger band_capacity on the second block.
     raw_copy_unpack's growth of d_raw[0]: sc8 (2 bytes per sample), then sc16 (4).
     sf_reserve_bits and the sync finder's segment counters: a short bit stream, a longer one, one long enough for the multi-pass form.
   Compared is everything a record defines, bit for bit (test_gpu_sample_format._record_equal).  The bytes a batch of this kind does
   not write (include/mfbank.h: the clip tags outside clipped fixed-shift batches, the sync fields without templates, symbol entries
   past a block's count) are whatever the allocation held, on either handle, and are left out.

B. A cycle that creates, uses and closes a handle with everything that allocates late switched on, plus a sync finder and a combiner,
   must return device memory to within the 32 MiB that test_gpu_configs.test_failed_create_frees_everything allows.  At N = 2^18 one
   leaked N-sized complex64 buffer per cycle is 2 MiB, 40 MiB after 20 cycles.  Buffers below about 1.6 MiB (32 MiB / 20) are not
   seen by this reading, nor is page-locked memory: those are covered by construction (no hipFree / hipHostFree / hipEventDestroy /
   hipStreamDestroy is written out in mfbank.hip or its parts any more) and by tools/leak_probe.py."""
import numpy as np
import pytest

from pycusdr_amd.mfbank import Combiner, MFBank, SyncFinder
from test_gpu_sample_format import _record_equal, _same_block

pytestmark = pytest.mark.gpu

LOG2N, N = 14, 1 << 14
OV = 1024
STRIDE = N - OV
K = dict(k_offset=800, k_len=400, spsym_min=8)


def _bank(log2n=LOG2N, M=2, taps=32, seed=0):
    """Filters with a short impulse response (segment path: batches run there), 8 shifts."""
    n = 1 << log2n
    rs = np.random.RandomState(seed)
    h = np.zeros((M, n), np.complex64)
    h[:, :taps] = rs.standard_normal((M, taps)) + 1j * rs.standard_normal((M, taps))
    bank = MFBank(log2n, 8, M)
    bank.set_filters(np.conj(np.fft.fft(h, axis=1)).astype(np.complex64))
    bank.set_shifts(list(range(8)))
    return bank


def _samples(n, seed):
    """Noise, a tone and a few interference bursts (the clip has something to do), as int16 (I, Q) rows below full scale."""
    rng = np.random.default_rng(seed)
    x = 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.5 * np.exp(2j * np.pi * (1.3 / N) * np.arange(n))
    for p in rng.integers(0, n - 40, 24):
        x[p:p + int(rng.integers(1, 40))] *= rng.uniform(3, 8)
    q = np.round(np.stack((x.real, x.imag), axis=1) * (32767 / np.abs(np.stack((x.real, x.imag))).max()))
    return q.astype(np.int16)


def _everything_on(bank, overlap):
    bank.set_batch_overlap(True)
    bank.set_sample_format('sc16')
    bank.set_device_snr(True)
    bank.set_peak_clip(4.5, overlap)
    bank.set_stream_stages(OV, 20, 10, 1000, bit_lut=np.array([0, 1], np.uint8))


def _batch(bank, nb, q, slot=0):
    """nb blocks of q on windows made for nb blocks, from a restarted clip chain and an empty stream tail."""
    w = bank.windows(nb, STRIDE)[slot]
    w[:] = q[:nb * STRIDE + OV]
    bank.restart_peak_clip()
    bank.stream_seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    bank.begin_blocks(slot, nb, source=('window', 'window2')[slot], **K)
    return bank.end_blocks_record(slot)


def test_a_grown_handle_equals_a_fresh_one_batches():
    q = _samples(8 * STRIDE + OV, 5)
    grown, fresh = _bank(), _bank()
    try:
        _everything_on(grown, OV // 2)
        for _ in range(3):                   # plain launches, the capture, the replay: the graphs exist before anything regrows
            _batch(grown, 1, q)
        _batch(grown, 1, q, slot=1)
        grown.set_peak_clip(4.5, OV)         # the chain's tail regrows
        for slot in (0, 1):
            _batch(grown, 3, q, slot)
        last = [_batch(grown, 8, q, slot) for slot in (0, 1)]
        _everything_on(fresh, OV)
        for slot in (0, 1):
            want = _batch(fresh, 8, q, slot)
            assert want.nb == 8 and want.stages and want.snr_means is not None and sum(len(c) for c in want.clipped) > 0
            _record_equal(last[slot], want, ('batch of 8', slot))       # (the clipped-peak indices of every block among the rest)
        # the grown handle is not worn out: the smaller batch once more, against the fresh handle's
        _record_equal(_batch(grown, 3, q), _batch(fresh, 3, q), 'batch of 3 after 8')
    finally:
        grown.close()
        fresh.close()


def test_a_grown_handle_equals_a_fresh_one_single_block():
    q = _samples(N, 6)
    x = (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(N)
    grown, fresh = _bank(), _bank()
    try:
        def three_ways(h):
            h.input[:] = x
            out = [h.receive_block(**K)]
            for slot in (0, 1):
                h.begin_block(slot, **K)
                out.append(h.end_block(slot))
            return out
        three_ways(grown)                        # at the default capacity: the record and both stagings as mfb_create made them
        for h in (grown, fresh):
            h.BAND_CAPACITY, h._blk = 8192, None
        for a, b in zip(three_ways(grown), three_ways(fresh)):
            _same_block(a, b, 'band_capacity 8192')
        # integer samples of 2, then 4 bytes: the input's staging buffer grows between the two blocks
        grown.set_sample_format('sc8')
        grown.input[:] = (q >> 8).astype(np.int8)
        grown.receive_block(**K)
        for h in (grown, fresh):
            h.set_sample_format('sc16')
            h.input[:] = q
        _same_block(grown.receive_block(**K), fresh.receive_block(**K), 'sc16 after sc8')
    finally:
        grown.close()
        fresh.close()


def test_a_grown_sync_finder_equals_a_fresh_one():
    rng = np.random.default_rng(8)
    tmpl = rng.integers(0, 2, 32).astype(np.int8) * 2 - 1
    thr = int((tmpl > 0).sum())          # score[i] = sum_t tmpl[t] * bits[i - t]: reached exactly where the stream holds the +1 taps' pattern
    streams = [rng.integers(0, 2, n).astype(np.uint8) for n in (200, 5000, 40000)]      # 40000 bits: 40 segments, the multi-pass form
    for s in streams:
        for p in range(64, s.size - 64, 500):
            s[p:p + 32] = tmpl[::-1] > 0                                                 # a certain hit at p + 31
    grown = SyncFinder([tmpl], [thr], max_hits=1024, max_bits=64)
    try:
        for s in streams:
            fresh = SyncFinder([tmpl], [thr], max_hits=1024, max_bits=1 << 16)
            try:
                (gi, gs), (fi, fs) = grown.find(s)[0], fresh.find(s)[0]
            finally:
                fresh.close()
            assert np.array_equal(gi, fi) and np.array_equal(gs, fs), s.size
            assert set(range(64 + 31, s.size - 64 + 31, 500)) <= set(fi.tolist()) and len(fi) <= 1024, s.size
    finally:
        grown.close()


# ---- B ---------------------------------------------------------------------------------------------------------------------------
B_LOG2N, B_CYCLES, B_SETTLE = 18, 20, 2


def _cycle(q, bits):
    n = 1 << B_LOG2N
    bank = _bank(B_LOG2N, M=4)
    try:
        bank.set_batch_overlap(True)
        bank.set_peak_clip(4.5, OV)
        w = bank.windows(4, n - OV)[0]
        w[:] = q[:w.size]
        bank.begin_blocks(0, 4, source='window', **K)
        assert bank.end_blocks_record(0).nb == 4
        bank.set_peak_clip(0)
        bank.upload(q[:n])
        bank.get_spectrum(0, 16)                 # from here on every spectrum is mirrored to the host on a stream of its own
        bank.upload(q[:n])
        bank.get_spectrum(0, 16)
        bank.set_search_mode('energy')
        bank.find_carrier()
        bank.set_search_mode('transforms')
        bank.set_search_basis('span')
        bank.find_carrier()
    finally:
        bank.close()
    sf = SyncFinder([np.ones(16, np.int8)], [12], max_bits=1 << 12)
    try:
        sf.find(bits)
    finally:
        sf.close()
    cmb = Combiner(max_bits=1 << 12, max_slaves=0)
    try:
        cmb.combine(bits[:4096], np.ones(4096, np.int8), [], 3.0, 16)
    finally:
        cmb.close()


def test_b_cycles_return_device_memory():
    import time
    import torch
    n = 1 << B_LOG2N
    assert B_CYCLES * n * 8 > (32 << 20)         # one N-sized complex64 buffer per cycle would cross the bound
    rng = np.random.default_rng(9)
    q = (rng.standard_normal(4 * (n - OV) + OV) + 1j * rng.standard_normal(4 * (n - OV) + OV)).astype(np.complex64)
    bits = rng.integers(0, 2, 6000).astype(np.uint8)
    for _ in range(B_SETTLE):
        _cycle(q, bits)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    for _ in range(B_CYCLES):
        _cycle(q, bits)
    per_cycle = (time.perf_counter() - t0) / B_CYCLES
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f'{B_CYCLES} cycles at 2^{B_LOG2N}: {per_cycle * 1e3:.1f} ms each, device free {free0 >> 20} -> {free1 >> 20} MiB')
    assert abs(free0 - free1) < (32 << 20), (free0, free1)
