"""Shared by test_combiner_host.py and test_gpu_combiner.py: the recorded scenarios of tests/golden/ref_goldens_combiner.npz
(made by tests/golden/make_golden_combiner.py from the reference's own SoftCombiner) and a runner for them."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_goldens_combiner.npz')
SCENARIOS = ['a_two_slaves', 'b_one_slave', 'c_second_slave_ends_early', 'd_below_minimum', 'e_one_unrelated', 'f_nothing_matched',
             'f_held_back', 'g_power_of_two_wrap', 'h_word_offsets_0_and_31', 'i_full_length', 'j_three_slaves', 'k_other_vote_group']
TRUST_REPS = [-128, -17, -2, -1, 0, 1, 127]
WEIGHTS = [1.2, 1.0, 0.8]


@functools.lru_cache(maxsize=1)
def goldens():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k.replace('__', '/'): z[k] for k in z.files}


def conf_of(min_length=200, variance_multiplier=15.0, weight=1.2, threshold=1):
    return {'SoftCombiner': {'processingInterval': 0.3, 'pollingTimeout': 95, 'workerTimeout': 20.0, 'workerDataTimeout': 1e9,
                             'varianceMultiplier': variance_multiplier, 'minProcessingLength': int(min_length),
                             'workerDataRequestThreshold': int(threshold), 'masterVoteWeight': weight}}


def scenario_inputs(name):
    """(conf, [worker dicts, master first])."""
    g = goldens()
    p = f'sc/{name}/'
    minlen, vm, weight, thr = g[p + 'conf']
    workers = []
    for i in range(int(g[p + 'nworkers'])):
        n = int(g[p + f'w{i}/len'])
        bits = np.unpackbits(g[p + f'w{i}/bits'])[:n].astype(np.int8)
        workers.append({'workerId': f'w{i}', 'count': 0, 'timestamp': 0.0, 'voteGroup': int(g[p + f'w{i}/voteGroup']), 'data': bits,
                        'trust': g[p + f'w{i}/trust']})
    return conf_of(minlen, vm, weight, thr), workers


def run_scenario(name, backend):
    """One correlate(master, slaves) call as recorded; returns (result or None, workers, combiner)."""
    from pycusdr_amd.softCombiner import SoftCombiner
    conf, dicts = scenario_inputs(name)
    comb = SoftCombiner(conf, backend=backend, clock=lambda: 0.0)
    ws = [comb.insert(d) for d in dicts]
    return comb.correlate(ws[0], ws[1:]), ws, comb


def check_against_reference(name, res, ws):
    """What the reference returned and left behind, byte for byte."""
    g = goldens()
    p = f'sc/{name}/'
    assert (res is None) == bool(g[p + 'none']), name
    if res is not None:
        assert res['data'].dtype == np.int8 and res['trust'].dtype == np.int8, name
        assert res['data'].tobytes() == g[p + 'data'].tobytes(), name
        assert res['trust'].tobytes() == g[p + 'trust'].tobytes(), name
        assert res['numSlaves'] == int(g[p + 'numSlaves']), name
        assert list(res['slaveNames']) == [str(s) for s in g[p + 'slaveNames']], name
        assert res['count'] == int(g[p + 'count']) and res['workerId'] == 'w0', name
    assert [w.head for w in ws] == list(g[p + 'head']), name
    assert [w.tail for w in ws] == list(g[p + 'tail']), name
    assert [w.getCount for w in ws] == list(g[p + 'getCount']), name
    assert [w.getDataRequestCounter() for w in ws] == list(g[p + 'requests']), name


def core_inputs(name):
    """The core's arguments of a scenario: master bits, trust and the (bits, trust) buffers of the slaves in its vote group."""
    _, dicts = scenario_inputs(name)
    group = [d for d in dicts[1:] if d['voteGroup'] == dicts[0]['voteGroup']]
    return dicts[0]['data'], dicts[0]['trust'], [(d['data'], d['trust']) for d in group]


def vote_inputs(voters):
    g = goldens()
    trust = g[f'vote/{voters}/in_trust']
    bits = np.unpackbits(g[f'vote/{voters}/in_bits'], axis=1)[:, :trust.shape[1]].astype(np.int8)
    return bits, trust


def same_core(a, b, cond_rel=0.0):
    """Two results of the core (Combiner.end's dict) agree; cond within cond_rel relative."""
    assert a['status'] == b['status'] and a['matched'] == b['matched']
    assert a['bits'].tobytes() == b['bits'].tobytes() and a['trust'].tobytes() == b['trust'].tobytes()
    assert len(a['slaves']) == len(b['slaves'])
    for ra, rb in zip(a['slaves'], b['slaves']):
        for k in ('evaluated', 'matched', 'idx0', 'avail', 'lc_after'):
            assert ra[k] == rb[k], (k, ra, rb)
        assert np.array_equal(ra['val'], rb['val']), (ra, rb)
        assert abs(ra['cond'] - rb['cond']) <= cond_rel * abs(rb['cond']), (ra['cond'], rb['cond'])
