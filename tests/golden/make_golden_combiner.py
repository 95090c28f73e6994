#!/usr/bin/env python3
"""Generate ``ref_goldens_combiner.npz`` from the reference's own soft combiner (pyCuSDR/softCombiner.py, mounted
read-only at /root/reference in the authoring container).

Test infrastructure, like make_golden.py: it runs only where the reference exists; its output is data (inputs and
recorded results) and is what tests/test_combiner_host.py and tests/test_gpu_combiner.py read.

The reference module is imported with ``zmq`` stubbed (as make_golden.py does for sigFIFO); ``SoftCombiner`` is a
``Process`` whose constructor wants sockets and a config tree, so the object is made with ``object.__new__`` and given
the four attributes ``correlate`` and the votes read.  ``Worker`` and ``correlate`` run unchanged.  The module's
``customXCorr`` is wrapped to keep every correlation the reference computed, from which the peaks and the decision
threshold are re-derived here with the reference's own steps (softCombiner.py:709-721) and recorded beside the outputs.

  sc/<name>/...   scenarios a .. j of one ``correlate(master, slaves)`` call each: the workers' bits and trust, the
                  configuration, what the call returned and every worker's indices afterwards
  vote/...        _doVote2 / _doVoteN over every column state of 2, 3 and 4 voters, bits {0, 1} x trust
                  {-128, -17, -2, -1, 0, 1, 127}, for masterVoteWeight 1.2, 1.0 and 0.8

The file is refused unless every recorded decision has |val[0] - cond| >= 1, every matched slave val[0] - val[1] >= 1
and every correlation value the reference saw lies within 1e-6 of an integer: the exact integer form is then
indistinguishable from the reference's float64 form on these streams.

Usage:  python tests/golden/make_golden_combiner.py
"""
import itertools
import os
import sys
import types

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
MIN_LEN, VAR_MULT = 200, 15.0
TRUST_REPS = [-128, -17, -2, -1, 0, 1, 127]
WEIGHTS = [1.2, 1.0, 0.8]


def import_reference():
    sys.modules['zmq'] = types.ModuleType('zmq')
    sys.path.insert(0, os.path.join(REF, 'pyCuSDR'))
    import softCombiner as ref
    return ref


def make_combiner(ref, weight=1.2, threshold=1):
    c = object.__new__(ref.SoftCombiner)
    c.MIN_LENGTH = MIN_LEN
    c.varMultiplier = VAR_MULT
    c.masterVoteWeight = weight
    c.dataRequestThreshold = threshold
    return c


def noisy(rs, bits, rate):
    b = np.array(bits, dtype=np.int8)
    flip = rs.random_sample(len(b)) < rate
    b[flip] ^= 1
    return b


def trust_for(rs, n):
    t = rs.randint(-3, 4, n)
    wild = rs.random_sample(n) < 0.1
    t[wild] = rs.randint(-128, 128, int(wild.sum()))
    return t.astype(np.int8)


def scenarios(base):
    """name -> (threshold, [(bits, trust, voteGroup) per worker, master first])."""
    rs = np.random.RandomState(20260)
    L = len(base)
    rnd = lambda n: rs.randint(0, 2, n).astype(np.int8)        # noqa: E731
    cut = lambda s, n, rate: noisy(rs, base[s:s + n], rate)    # noqa: E731
    sc = {}
    sc['a_two_slaves'] = (1, [cut(2000, 3001, .02), cut(1500, 4999, .03), cut(1000, 5003, .05)])
    sc['b_one_slave'] = (1, [cut(7000, 2113, .02), cut(6400, 4001, .04)])
    sc['c_second_slave_ends_early'] = (1, [cut(12000, 3001, .02), cut(11500, 4999, .03), cut(11000, 3503, .03)])
    # d, g: a slave buffer of exactly a power of two bits and a master that runs round its end: the correlation is circular
    s = cut(20000, 1024, 0.)
    sc['d_below_minimum'] = (1, [noisy(rs, np.roll(s, -874)[:1000], .02), noisy(rs, s, .02)])
    s = cut(22000, 2048, 0.)
    sc['g_power_of_two_wrap'] = (1, [np.r_[noisy(rs, np.roll(s, -(2047 - 5)), .02), rnd(453)], noisy(rs, s, .02)])
    sc['e_one_unrelated'] = (1, [cut(30000, 2999, .02), rnd(4001), cut(29000, 5001, .03)])
    sc['f_nothing_matched'] = (1, [cut(33000, 1999, .02), rnd(3001), rnd(2501)])
    sc['f_held_back'] = (3, [cut(33000, 1999, .02), rnd(3001), rnd(2501)])
    sc['h_word_offsets_0_and_31'] = (1, [cut(40000, 2001, .02), cut(40000 - 512, 4001, .03), cut(40000 - 543, 4003, .03)])
    sc['i_full_length'] = (1, [cut(30000, 5999, .02), noisy(rs, base, .03)])
    sc['j_three_slaves'] = (1, [cut(50000, 2501, .02), cut(49000, 4501, .03), cut(48500, 5001, .04), cut(49900, 3001, .05)])
    sc['k_other_vote_group'] = (1, [cut(52000, 1501, .02), cut(51500, 3001, .03), cut(51000, 3001, .03)])
    out = {}
    for name, (thr, streams) in sc.items():
        assert all(len(b) <= L for b in streams)
        groups = [0] * len(streams)
        if name == 'k_other_vote_group':
            groups[1] = 1                  # the first slave belongs to another vote group and is never looked at
        out[name] = (thr, [(b, trust_for(rs, len(b)), g) for b, g in zip(streams, groups)])
    return out


def run_scenario(ref, name, thr, workers, out):
    comb = make_combiner(ref, 1.2, thr)
    seen = []
    real = ref.customXCorr

    def spy(a, b, N=None):
        r = real(a, b, N)
        seen.append(np.abs(r))
        return r
    ref.customXCorr = spy
    try:
        ws = [ref.Worker({'workerId': f'w{i}', 'count': 0, 'timestamp': 0.0, 'voteGroup': g, 'data': b, 'trust': t}, timestampTimeOut=1e9)
              for i, (b, t, g) in enumerate(workers)]
        res = comb.correlate(ws[0], ws[1:])
    finally:
        ref.customXCorr = real
    vals, idx0s, conds = [], [], []
    for x in seen:
        assert np.abs(x - np.rint(x)).max() < 1e-6, name
        x = x.copy()
        idx = np.empty(15, dtype=int)
        val = np.empty(15)
        for i in range(15):
            idx[i] = np.argmax(x)
            val[i] = x[idx[i]]
            x[idx[i]] = 0
        cond = np.mean(val[2:]) + VAR_MULT * np.std(val[2:])
        assert abs(val[0] - cond) >= 1, (name, val[0], cond)
        if val[0] > cond:
            assert val[0] - val[1] >= 1, (name, val[:2])
        vals.append(np.rint(val).astype(np.int32))
        idx0s.append(idx[0])
        conds.append(cond)
        print(f'  {name}: val0 {val[0]:.0f} val1 {val[1]:.0f} cond {cond:.1f} idx0 {idx[0]} matched {val[0] > cond}')
    p = f'sc/{name}/'
    out[p + 'conf'] = np.array([MIN_LEN, VAR_MULT, 1.2, thr], dtype=np.float64)
    out[p + 'nworkers'] = np.int64(len(workers))
    for i, (b, t, g) in enumerate(workers):
        out[p + f'w{i}/bits'] = np.packbits(b.astype(np.uint8))
        out[p + f'w{i}/len'] = np.int64(len(b))
        out[p + f'w{i}/trust'] = t
        out[p + f'w{i}/voteGroup'] = np.int64(g)
    out[p + 'ref_val'] = np.array(vals, dtype=np.int32).reshape(-1, 15)
    out[p + 'ref_idx0'] = np.array(idx0s, dtype=np.int64)
    out[p + 'ref_cond'] = np.array(conds, dtype=np.float64)
    out[p + 'none'] = np.bool_(res is None)
    if res is not None:
        out[p + 'data'] = np.asarray(res['data']).astype(np.int8)
        out[p + 'trust'] = np.asarray(res['trust']).astype(np.int8)
        assert np.asarray(res['data']).dtype == np.int8 and np.asarray(res['trust']).dtype == np.int8
        out[p + 'numSlaves'] = np.int64(res['numSlaves'])
        out[p + 'slaveNames'] = np.array(res['slaveNames'], dtype='U8')
        out[p + 'count'] = np.int64(res['count'])
    out[p + 'head'] = np.array([w.head for w in ws], dtype=np.int64)
    out[p + 'tail'] = np.array([w.tail for w in ws], dtype=np.int64)
    out[p + 'getCount'] = np.array([w.getCount for w in ws], dtype=np.int64)
    out[p + 'requests'] = np.array([w.getDataRequestCounter() for w in ws], dtype=np.int64)
    print(f'{name}: ' + ('None' if res is None else f"{len(res['data'])} bits, slaves {res['slaveNames']}"))


def vote_columns(voters):
    """Every column state: (bits [voters, C], trust [voters, C]), voter 0 the master, the master's state varying fastest."""
    per = [(b, t) for b in (0, 1) for t in TRUST_REPS]
    cols = list(itertools.product(range(len(per)), repeat=voters))
    bits = np.array([[per[c[voters - 1 - v]][0] for c in cols] for v in range(voters)], dtype=np.int8)
    trust = np.array([[per[c[voters - 1 - v]][1] for c in cols] for v in range(voters)], dtype=np.int8)
    return bits, trust


def votes(ref, out):
    for voters in (2, 3, 4):
        bits, trust = vote_columns(voters)
        out[f'vote/{voters}/in_bits'] = np.packbits(bits.astype(np.uint8), axis=1)
        out[f'vote/{voters}/in_trust'] = trust
        for w in WEIGHTS:
            comb = make_combiner(ref, w)
            if voters == 2:
                b, t = comb._doVote2(bits[0].copy(), trust[0].copy(), bits[1].copy(), trust[1].copy())
            else:
                b, t = comb._doVoteN(bits[0].copy(), trust[0].copy(), [r.copy() for r in bits[1:]], [r.copy() for r in trust[1:]])
            assert b.dtype == np.int8 and t.dtype == np.int8 and set(np.unique(b)) <= {0, 1}
            out[f'vote/{voters}/w{w}/bits'] = b
            out[f'vote/{voters}/w{w}/trust'] = t
        print(f'vote {voters}: {bits.shape[1]} columns')


def main():
    ref = import_reference()
    z = np.load(os.path.join(REF, 'test', 'test_trustProcessor', 'bitData_test.npz'))
    base = np.asarray(z['ddR1']).astype(np.int8)
    assert len(base) == 58834 and set(np.unique(base)) <= {0, 1}
    out = {}
    for name, (thr, workers) in scenarios(base).items():
        run_scenario(ref, name, thr, workers, out)
    votes(ref, out)
    path = os.path.join(HERE, 'ref_goldens_combiner.npz')
    np.savez_compressed(path, **{k.replace('/', '__'): v for k, v in out.items()})
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
