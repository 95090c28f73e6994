"""The soft combiner's host back end (pycusdr_amd/softCombiner.py) against recordings of the reference's own SoftCombiner
(tests/golden/ref_goldens_combiner.npz): no GPU."""
import numpy as np
import pytest

import combiner_common as cc
from pycusdr_amd import softCombiner as sc


@pytest.mark.parametrize('name', cc.SCENARIOS)
def test_scenario_equals_the_reference(name):
    """Status, numSlaves, slaveNames, bits and trust byte for byte; every worker's head / tail and counters afterwards; and the
    exact integer peaks, their lag and the threshold against what the reference's float64 FFT form gave."""
    res, ws, comb = cc.run_scenario(name, 'host')
    cc.check_against_reference(name, res, ws)
    g = cc.goldens()
    core = comb.combine(*cc.core_inputs(name))
    evaluated = [r for r in core['slaves'] if r['evaluated']]
    assert len(evaluated) == len(g[f'sc/{name}/ref_idx0'])
    for r, val, idx0, cond in zip(evaluated, g[f'sc/{name}/ref_val'], g[f'sc/{name}/ref_idx0'], g[f'sc/{name}/ref_cond']):
        assert np.array_equal(r['val'], val) and r['idx0'] == idx0
        assert abs(r['cond'] - cond) <= 1e-9 * cond
    assert comb.host_fallbacks == 0


@pytest.mark.parametrize('voters', [2, 3, 4])
def test_vote_and_tables_equal_the_exhaustive_recordings(voters):
    """_doVote2 / _doVoteN over every column state (bits x trust representatives of every class and both extremes): the
    numpy form and the table the device votes with give the recorded bit and trust byte, for all three weights."""
    g = cc.goldens()
    bits, trust = cc.vote_inputs(voters)
    assert bits.shape == (voters, 14 ** voters)
    states = sc.column_states(list(bits), list(trust))
    assert len(np.unique(states)) == 8 ** voters           # the recordings reach every table entry
    for w in cc.WEIGHTS:
        rb, rt = g[f'vote/{voters}/w{w}/bits'], g[f'vote/{voters}/w{w}/trust']
        if voters == 2:
            b, t = sc.vote2(bits[0], trust[0], bits[1], trust[1])
        else:
            b, t = sc.voteN(bits[0], trust[0], list(bits[1:]), list(trust[1:]), w)
        assert b.dtype == np.int8 and t.dtype == np.int8
        assert np.array_equal(b, rb) and np.array_equal(t, rt), w
        tb, tt = sc.vote_table(voters, w)
        assert tb.shape == tt.shape == (8 ** voters,) and tb.dtype == np.uint8 and tt.dtype == np.int8
        assert np.array_equal(tb[states], rb.astype(np.uint8)) and np.array_equal(tt[states], rt), w


def test_host_core_votes_through_tables_alike():
    """combine_host with the tables (what the device does) equals combine_host with the vote functions."""
    for name in ('a_two_slaves', 'b_one_slave', 'j_three_slaves'):
        m, t, slaves = cc.core_inputs(name)
        tables = {v: sc.vote_table(v, 1.2) for v in (2, 3, 4)}
        cc.same_core(sc.combine_host(m, t, slaves, 15.0, 1.2, 200, tables=tables), sc.combine_host(m, t, slaves, 15.0, 1.2, 200))


def test_bit_xcorr_host_is_the_definition():
    rs = np.random.RandomState(3)
    for n, m in ((16, 5), (37, 64), (64, 64), (100, 31)):
        a, b = rs.randint(0, 2, n), rs.randint(0, 2, m)
        N = sc.pow2ceil(n)
        ap = np.r_[a, np.zeros(N - n, dtype=int)]
        L = min(n, m)
        want = [sum(ap[(j + k) % N] * b[j] for j in range(L)) for k in range(N)]
        assert list(sc.bit_xcorr_host(a, b)) == want
    val, idx0 = sc.top_peaks([3, 9, 9, 0, 1])
    assert list(val[:5]) == [9, 9, 3, 1, 0] and idx0 == 1 and len(val) == 15


def test_short_slaves_are_not_evaluated():
    """The documented deviation: a slave buffer of fewer than 16 bits is never matched (the reference would raise)."""
    m, t, slaves = cc.core_inputs('b_one_slave')
    tiny = (np.ones(15, np.int8), np.zeros(15, np.int8))
    res = sc.combine_host(m, t, [tiny] + slaves, 15.0, 1.2, 200)
    assert res['slaves'][0]['evaluated'] == 0 and res['matched'] == [1] and res['status'] == sc.COMBINED
    cc.same_core({**res, 'slaves': res['slaves'][1:], 'matched': [0]}, sc.combine_host(m, t, slaves, 15.0, 1.2, 200))


def test_worker_bookkeeping_under_a_fake_clock():
    now = [0.0]
    w = sc.Worker({'workerId': 'a', 'count': 0, 'voteGroup': 2, 'SNR': '7.5', 'data': [1, 0, 1], 'trust': [1, 2, 3]}, timestampTimeOut=1.0,
                  clock=lambda: now[0])
    assert (w.head, w.tail, w.voteGroup, w.data['SNR']) == (0, 3, 2, 7.5) and w.data['data'].dtype == np.int8
    now[0] = 0.5
    w.insertData({'workerId': 'a', 'count': 1, 'data': [0, 0, 1, 1], 'trust': [-1, -2, 0, 5]})
    assert (w.head, w.tail) == (0, 7) and w.arrivalTimes == [{'time': 0.0, 'idx': 0}, {'time': 0.5, 'idx': 3}]
    out = w.getSelf()
    assert list(out['data']) == [1, 0, 1, 0, 0, 1, 1] and list(out['trust']) == [1, 2, 3, -1, -2, 0, 5]
    assert (out['workerId'], out['count'], out['voteGroup'], out['doppler']) == ('a', 0, 2, [])
    assert (w.head, w.getCount, w.totalRequestCount, w.getDataRequestCounter()) == (7, 1, 1, 1)
    out = w.getSelf()                      # nothing new: no counter moves, the block number is the next one
    assert len(out['data']) == 0 and out['count'] == 1 and (w.getCount, w.getDataRequestCounter()) == (1, 1)
    w.updateIdx(2)                         # two bits handed back (a truncation)
    out = w.getSelf()
    assert list(out['data']) == [1, 1] and (w.head, w.getCount, w.getDataRequestCounter()) == (7, 2, 2)
    w.updateIdx(2, dataUsed=False)         # handed back unused
    assert (w.head, w.getCount) == (5, 1)
    w.clearDataRequestCounter()
    assert w.getDataRequestCounter() == 0 and w.totalRequestCount == 2
    now[0] = 1.2                           # the first block (arrived at 0) is older than 1 s, the second is not
    w.removeOldData()
    assert list(w.data['data']) == [0, 0, 1, 1] and (w.head, w.tail) == (2, 4) and w.arrivalTimes == [{'time': 0.5, 'idx': 0}]
    now[0] = 5.0
    w.insertData({'workerId': 'a', 'count': 2, 'data': [1, 1], 'trust': [0, 0]})
    w.removeOldData()                      # drops four bits although only two were handed on: the head stops at 0
    assert list(w.data['data']) == [1, 1] and (w.head, w.tail) == (0, 2) and w.arrivalTimes == [{'time': 5.0, 'idx': 0}]
    now[0] = 100.0
    w.removeOldData()                      # the newest block always stays
    assert (w.head, w.tail) == (0, 2) and len(w.data['trust']) == 2
    assert len(w.getData()[0]) == 2 and list(w.getData(1)[0]) == [1]
    with pytest.raises(IndexError):
        w.getData(2)
    with pytest.raises(sc.WorkerIdError):
        w.insertData({'workerId': 'b', 'count': 3, 'data': [1], 'trust': [0]})


def test_compare_workers_takes_every_worker_as_master():
    """compareWorkers: every worker is the master once.  w0's new bits lie inside both other buffers: one dict with numSlaves /
    slaveNames.  The new bits of w1 and w2 begin before w0's buffer does: the lag wraps round, the slice holds nothing, and
    they are handed back (head 0 again) and tried again next round.  Data older than workerDataTimeout is dropped afterwards."""
    now = [0.0]
    _, dicts = cc.scenario_inputs('a_two_slaves')
    conf = cc.conf_of()
    conf['SoftCombiner']['workerDataTimeout'] = 3.5
    comb = sc.SoftCombiner(conf, backend='host', clock=lambda: now[0])
    for d in dicts:
        comb.insert(d)
    out = comb.compareWorkers()
    assert [d['workerId'] for d in out] == ['w0']
    assert [(w.head, w.getCount) for w in comb.workers] == [(3001, 1), (0, 0), (0, 0)]
    assert out[0]['numSlaves'] == 2 and out[0]['slaveNames'] == ['w1', 'w2']
    assert out[0]['data'].tobytes() == cc.goldens()['sc/a_two_slaves/data'].tobytes()
    assert comb.compareWorkers() == []
    now[0] = 1.0
    comb.insert({**dicts[0], 'count': 1})
    now[0] = 4.0
    comb.compareWorkers()
    assert len(comb.workers[0].data['data']) == len(dicts[0]['data']) and comb.workers[0].arrivalTimes[0]['idx'] == 0


def test_binding_carries_the_new_symbols():
    from pycusdr_amd import _lib
    for name in ('mfb_combiner_create', 'mfb_combiner_destroy', 'mfb_combiner_set_vote', 'mfb_combiner_begin', 'mfb_combiner_end',
                 'mfb_debug_bit_xcorr', 'mfb_debug_combine_peaks'):
        assert name in _lib.PROTOTYPES
    import ctypes
    assert ctypes.sizeof(_lib.CombineSlave) == 96 and ctypes.sizeof(_lib.CombineResult) == 320 and ctypes.sizeof(_lib.CombineParams) == 32
