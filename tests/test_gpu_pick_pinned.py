"""The pick's two floats reach the host without a copy: k_pick stores them into the handle's page-locked result slot itself and
mfb_pick / mfb_pick_column / mfb_find_carrier read the slot after synchronising the stream (no hipMemcpyAsync behind the kernel).
The values are pick_body's, untouched: every way of asking for the pick of one table gives the same bits -- find_carrier, pick on the
handle's own table, pick on a device copy of the table that get_scores returned, and pick_column on its column 0 --, the index is the
oracle's on that table, and a slot belongs to one handle: picks back to back and picks from two threads on two handles each read their
own value.  D = 2, 64, 65 and 256 (one wave's rows, one more, several chunks) on one 2^15-sample block, without and with the
noise-reference bin in front of the table (doppler_offset 0 and 1)."""
import threading

import numpy as np
import pytest

from oracle import mfbank_oracle as orc

pytestmark = pytest.mark.gpu

LOG2N, M = 15, 4
N = 1 << LOG2N
CASES = [(D, doff) for D in (2, 64, 65, 256) for doff in (0, 1)]


def _rand_c64(rs, *shape):
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)


@pytest.fixture(scope='module')
def block():
    rs = np.random.RandomState(14)
    return {'x': _rand_c64(rs, N), 'masks': _rand_c64(rs, M, N), 'shifts': rs.randint(0, N, 257).astype(np.int32)}


def _bank(block, D, doff):
    from pycusdr_amd.mfbank import MFBank
    bank = MFBank(LOG2N, D, M, sum_all_masks=True, doppler_offset=doff)
    bank.set_filters(block['masks'])
    bank.set_shifts(block['shifts'][:D + doff])
    return bank


def _bits(pick):
    return np.asarray(pick, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize('D,doff', CASES)
def test_every_way_to_the_pick_of_one_table_gives_the_same_bits(block, D, doff):
    import torch
    bank = _bank(block, D, doff)
    try:
        bank.upload(block['x'])
        found = bank.find_carrier()
        table = bank.get_scores()
        own = bank.pick()
        dev = torch.from_numpy(table).to('cuda:0')
        col = torch.from_numpy(np.ascontiguousarray(table[:, 0])).to('cuda:0')
        torch.cuda.synchronize()
        ref = bank.pick(dev.data_ptr(), D, doff)           # the reference: mfb_pick on a device copy of the table
        column = bank.pick_column(col.data_ptr(), D, doff)
        again = bank.find_carrier()
    finally:
        bank.close()
    assert table.shape == (D + doff, M) and np.isfinite(ref[0]) and np.isfinite(ref[1])
    for name, got in (('find_carrier', found), ('pick', own), ('pick_column', column), ('find_carrier, second call', again)):
        assert _bits(got) == _bits(ref), (name, got, ref)
    oidx, ometric = orc.find_doppler_est(table, D, doff, True)
    assert ref[0] == oidx
    assert abs(float(ref[1]) - float(ometric)) <= 2e-6 * abs(float(ometric)) + 1e-6


def _tables(rs, D, doff, count):
    """count tables [D + doff][M] with their maxima at different rows, column 0 populated (SUM_ALL_MASKS)"""
    out = []
    for i in range(count):
        t = np.zeros((D + doff, M), dtype=np.float32)
        t[:, 0] = 1.0 + rs.random_sample(D + doff).astype(np.float32)
        t[doff + (7 * i + 3) % D, 0] = 10.0 + i
        out.append(t)
    return out


def test_two_picks_back_to_back_on_one_handle_each_read_their_own_value(block):
    import torch
    D, doff = 65, 1
    tabs = _tables(np.random.RandomState(3), D, doff, 2)
    want = [orc.find_doppler_est(t, D, doff, True)[0] for t in tabs]
    assert want[0] != want[1]
    dev = [torch.from_numpy(t).to('cuda:0') for t in tabs]
    torch.cuda.synchronize()
    bank = _bank(block, D, doff)
    try:
        got = [bank.pick(dev[i % 2].data_ptr(), D, doff) for i in range(6)]
    finally:
        bank.close()
    for i, g in enumerate(got):
        assert g[0] == want[i % 2], (i, g, want)
        assert _bits(g) == _bits(got[i % 2]), i


def test_two_handles_in_two_threads_each_read_their_own_value(block):
    import torch
    D, doff, rounds = 64, 0, 50
    tabs = _tables(np.random.RandomState(4), D, doff, 2)
    want = [orc.find_doppler_est(t, D, doff, True)[0] for t in tabs]
    assert want[0] != want[1]
    dev = [torch.from_numpy(t).to('cuda:0') for t in tabs]
    torch.cuda.synchronize()
    banks = [_bank(block, D, doff) for _ in range(2)]
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(rounds):
                got[k].append(banks[k].pick(dev[k].data_ptr(), D, doff))
        except Exception as e:                               # noqa: BLE001 -- reported below, in the test's own thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads)
    finally:
        for b in banks:
            b.close()
    assert not errors, errors
    for k in range(2):
        assert len(got[k]) == rounds
        assert all(g[0] == want[k] and _bits(g) == _bits(got[k][0]) for g in got[k]), (k, want[k], got[k][:3])
