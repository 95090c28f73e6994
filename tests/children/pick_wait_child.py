"""Child of tests/test_gpu_pick_wait.py: picks taken from the handle's page-locked slot when they arrive (read_pick in csrc/bank_search_api.hpp),
not after a synchronise.  Two 2^15-sample blocks stay resident on the device; block b's spectrum sits in the band that bin CARRIER[b]
of the table shifts onto the filters' band, on a noise floor, so the two carriers lie 20 bins apart.  Every assertion is made here;
the parent runs a mode under a timeout.
usage: pick_wait_child.py alternate|threads|between"""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import mfbank_oracle as orc                                                # noqa: E402
from pycusdr_amd.mfbank import MFBank                                                  # noqa: E402

LOG2N, M, D, BAND = 15, 4, 64, 64
N = 1 << LOG2N
CARRIER = (17, 37)
CALLS = 300


def _setup():
    import torch
    rs = np.random.RandomState(29)
    masks = np.zeros((M, N), dtype=np.complex64)
    masks[:, :BAND] = rs.standard_normal((M, BAND)) + 1j * rs.standard_normal((M, BAND))
    shifts = (np.arange(D) * (N // D)).astype(np.int32)
    blocks = []
    for b in CARRIER:
        X = np.zeros(N, dtype=np.complex128)
        X[shifts[b]:shifts[b] + BAND] = rs.standard_normal(BAND) + 1j * rs.standard_normal(BAND)
        x = np.fft.ifft(X) * np.sqrt(N) + 1e-3 * (rs.standard_normal(N) + 1j * rs.standard_normal(N))
        blocks.append(np.asarray(x, dtype=np.complex64))
    dev = [torch.from_numpy(x).to('cuda:0') for x in blocks]
    torch.cuda.synchronize()
    return masks, shifts, blocks, dev


def _bank(masks, shifts):
    bank = MFBank(LOG2N, D, M, sum_all_masks=True)
    bank.set_filters(masks)
    bank.set_shifts(shifts)
    return bank


def _bits(pick):
    return np.asarray(pick, dtype=np.float32).view(np.uint32).tolist()


def _own(bank, dev):
    """(pick, table) of each block, taken one at a time with the table read back behind it; the picks are the oracle's on the table"""
    out = []
    for b, d in enumerate(dev):
        bank.upload_device(d.data_ptr())
        pick = bank.find_carrier()
        table = bank.get_scores()
        oidx, _ = orc.find_doppler_est(table, D, 0, True)
        assert pick[0] == oidx and abs(float(pick[0]) - CARRIER[b]) < 0.5, (b, pick, oidx)
        out.append((pick, table))
    assert abs(float(out[1][0][0]) - float(out[0][0][0]) - 20.0) < 1.0
    return out


def alternate():
    masks, shifts, _, dev = _setup()
    bank = _bank(masks, shifts)
    try:
        own = _own(bank, dev)
        for i in range(CALLS):
            bank.upload_device(dev[i % 2].data_ptr())
            got = bank.find_carrier()
            assert _bits(got) == _bits(own[i % 2][0]), (i, got, own[i % 2][0])      # a stale slot would hold the other block's
        # the table behind a pick is the table the pick was made on
        for b in (0, 1, 1, 0):
            bank.upload_device(dev[b].data_ptr())
            got = bank.find_carrier()
            assert np.array_equal(bank.get_scores(), own[b][1]) and _bits(got) == _bits(own[b][0]), b
    finally:
        bank.close()


def threads():
    masks, shifts, _, dev = _setup()
    banks = [_bank(masks, shifts) for _ in range(2)]
    errors = []

    def work(k):
        try:
            own = _own(banks[k], dev)
            for i in range(CALLS):
                b = (i + k) % 2
                banks[k].upload_device(dev[b].data_ptr())
                got = banks[k].find_carrier()
                assert _bits(got) == _bits(own[b][0]), (k, i, got, own[b][0])
        except BaseException as e:                           # noqa: BLE001 -- reported below, in the main thread
            errors.append((k, repr(e)))

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    try:
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ts)
    finally:
        for b in banks:
            b.close()
    assert not errors, errors


def between():
    import torch
    masks, shifts, _, dev = _setup()
    bank = _bank(masks, shifts)
    try:
        own = _own(bank, dev)
        rs = np.random.RandomState(5)
        tab = np.zeros((D, M), dtype=np.float32)
        tab[:, 0] = 1.0 + rs.random_sample(D).astype(np.float32)
        tab[50, 0] = 12.0
        want = orc.find_doppler_est(tab, D, 0, True)[0]
        dtab = torch.from_numpy(tab).to('cuda:0')
        dcol = torch.from_numpy(np.ascontiguousarray(tab[:, 0])).to('cuda:0')
        torch.cuda.synchronize()
        for i in range(20):
            b = i % 2
            bank.upload_device(dev[b].data_ptr())
            assert _bits(bank.find_carrier()) == _bits(own[b][0]), i
            p = bank.pick(dtab.data_ptr(), D, 0)
            c = bank.pick_column(dcol.data_ptr(), D, 0)
            assert p[0] == want and _bits(c) == _bits(p), (i, p, c, want)
            assert _bits(bank.pick()) == _bits(own[b][0]), i              # the handle's own table again
            bank.upload_device(dev[1 - b].data_ptr())
            assert _bits(bank.find_carrier()) == _bits(own[1 - b][0]), i
    finally:
        bank.close()


if __name__ == '__main__':
    {'alternate': alternate, 'threads': threads, 'between': between}[sys.argv[1]]()
    print('ok', sys.argv[1])
