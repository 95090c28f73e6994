"""The plain references of tests/combiner_model.py against the definition, the host back end and numpy itself: no GPU.  What
test_gpu_combiner_kernels.py holds the kernels to is only as good as these."""
import numpy as np
import pytest

import combiner_common as cc
import combiner_model as cm
from pycusdr_amd import softCombiner as sc


def test_exact_xcorr_is_the_definition_around_one_word():
    """Every slave length from one bit to beyond a word against master lengths around the word borders, shorter and longer
    than the slave: the big-integer form equals the definition's loops."""
    rs = np.random.RandomState(101)
    for n in range(1, 41):
        a = rs.randint(0, 2, n)
        for m in (1, 2, 15, 16, 17, 31, 32, 33, 64):
            b = rs.randint(0, 2, m)
            got = cm.exact_xcorr(a, b)
            assert got.dtype == np.int64 and got.shape == (cm.pow2ceil(n),)
            assert np.array_equal(got, cm.xcorr_by_definition(a, b)), (n, m)


def test_exact_xcorr_equals_the_host_back_end_at_a_long_shape():
    """(131 073, 70 000): N = 2^18, and the rounded float64 FFT form of the host back end gives the same integers."""
    rs = np.random.RandomState(102)
    a, b = rs.randint(0, 2, 131073), rs.randint(0, 2, 70000)
    assert np.array_equal(cm.exact_xcorr(a, b), sc.bit_xcorr_host(a, b))


def _descending_vectors(rs):
    """Fifteen peak values as the top-15 hands them over (descending, non-negative), 21 000 of them: values up to 2^20, small values
    with many ties, and all-equal vectors."""
    out = [np.sort(rs.randint(0, hi + 1, (3000, 15)), axis=1)[:, ::-1] for hi in (1 << 20, 70000, 1000, 40, 3, 1)]
    out.append(np.repeat(rs.randint(0, (1 << 20) + 1, (1500, 1)), 15, axis=1))
    out.append(np.repeat(np.arange(1500).reshape(-1, 1), 15, axis=1))
    return np.concatenate(out)


def test_decision_exact_is_numpy_bit_for_bit():
    rs = np.random.RandomState(103)
    vecs = _descending_vectors(rs)
    assert len(vecs) >= 20000
    for vm in (15.0, 3.7, 0.1):
        for v in vecs:
            want = sc.decision(v, vm)
            got = cm.decision_exact(v, vm)
            assert got[0] == want[0] and got[1] == want[1], (list(v), vm, got, want)
    flat = cm.decision_exact([7] * 15, 15.0)
    assert flat == (7.0, False)


@pytest.mark.parametrize('name', cc.SCENARIOS)
def test_decide_state_follows_combine_host(name):
    """Slave by slave through every recorded scenario: matched, avail, the master's length afterwards, cond and the call's
    status as combine_host gives them."""
    conf, _ = cc.scenario_inputs(name)
    vm, minlen = conf['SoftCombiner']['varianceMultiplier'], conf['SoftCombiner']['minProcessingLength']
    m, t, slaves = cc.core_inputs(name)
    res = sc.combine_host(m, t, slaves, vm, conf['SoftCombiner']['masterVoteWeight'], minlen)
    Lc, statuses = len(m), []
    for (b, _), rec in zip(slaves, res['slaves']):
        if not rec['evaluated']:
            continue
        st = cm.decide_state(rec['val'], rec['idx0'], len(b), Lc, minlen, vm)
        assert (st['matched'], st['avail'], st['lc_after']) == (rec['matched'], rec['avail'], rec['lc_after']), (name, st, rec)
        assert st['cond'] == rec['cond']
        Lc = st['lc_after']
        statuses.append(st['status'])
    want = cm.NOTHING if cm.NOTHING in statuses else cm.COMBINED if cm.COMBINED in statuses else cm.MASTER_ONLY
    assert (cm.NOTHING, cm.COMBINED, cm.MASTER_ONLY) == (sc.NOTHING, sc.COMBINED, sc.MASTER_ONLY)
    assert res['status'] == want and (res['status'] == sc.NOTHING or len(res['bits']) == Lc)
