"""The 256-point search with the wrap-around energy on the matrix cores (wrap_kernels.hpp, k_segw) on every bank, shape and call path
that reaches it -- not the bench_GMSK headline alone (tests/test_gpu_wrap_mfma.py): a seeded sweep of synthetic banks against the fp64
oracle (tests/tools/fuzz_wrap.py), the other shipped 48-tap banks, the span basis, batches of blocks, exact power-of-two scaling of
the input, and handles whose shifts, filters and basis change while they live.

Which form scores a block is ``seg_model.wrap_form``, a restatement of wrap_kt (csrc/search_plan.hpp); where it says 'matrix' the tables of
the two settings of MFB_SEG_WRAP_MFMA must differ, where it says 'vector' they must be bit-equal.  MFB_SEG_WRAP_MFMA is read once
per process: each form runs in a child of its own, every child under a time limit, and a child that fails ends the test."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mfbank_oracle as orc
from seg_model import filter_support, wrap_form

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, 'children', 'wrap_child.py')
CALLS = os.path.join(HERE, 'children', 'wrap_calls_child.py')
sys.path.insert(0, os.path.join(HERE, 'tools'))

pytestmark = pytest.mark.gpu

LOG2N = 18
N = 1 << LOG2N


def _env(form):
    env = dict(os.environ, MFB_SEG_WRAP_MFMA=form)
    for k in ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP'):
        env.pop(k, None)
    return env


def _same(a, b):
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


# ---- 1. the seeded sweep -----------------------------------------------------------------------------------------------------------
def test_sweep_of_both_forms_against_the_oracle(tmp_path):
    """tests/tools/fuzz_wrap.py, once per form with the same seed.  Per case and basis: both forms within 1e-5 of the oracle relative to
    the table's largest score, with the pick the oracle's scan of the device's own table gives (fuzz_seg.py's rules, no bin left
    out); on noise inputs the matrix form per bin no further from the oracle than twice the vector form plus 2e-7; the form that ran,
    from the two runs' bits, is the one ``wrap_form`` names -- 33 and 49 taps on the vector form, 34 and 48 on the matrix form --; and
    at least half of the cases took the matrix form."""
    import fuzz_wrap as fw
    valu = fw.run_form('0', str(tmp_path / 'sweep0.npz'))
    mfma = fw.run_form('1', str(tmp_path / 'sweep1.npz'))
    s = fw.check(valu, mfma)
    print(fw.summary_line(s))
    assert s['cases'] == fw.CASES
    assert 2 * s['matrix_cases'] >= s['cases'], s
    assert s['worst']['matrix'] > 0 and s['worst']['vector'] > 0


# ---- 2. the shipped banks, the span basis ----------------------------------------------------------------------------------------------
def _masks(name, log2N=LOG2N, D=64):
    from pycusdr_amd import config as cfg
    from pycusdr_amd.protocol import loadProtocol
    conf = cfg.bench_config(name, blockSize=log2N, doppCarrierSteps=D)
    _, masks = loadProtocol(name)(conf=conf).get_filter(1 << log2N, 16, 3)
    return np.asarray(masks)


_runs = {}


def _bank_run(name, tmp_path_factory):
    """(vector-form child, matrix-form child, oracle table per input) of ``name`` at 2^18 x 64 bins, default and span basis; once per
    session"""
    if name not in _runs:
        d = tmp_path_factory.mktemp(name)
        res = {}
        for form in ('0', '1'):
            out = str(d / f'wrap{form}.npz')
            subprocess.run([sys.executable, CHILD, name, str(LOG2N), '64', out, 'span'], check=True, env=_env(form), timeout=600)
            res[form] = dict(np.load(out))
        valu, mfma = res['0'], res['1']
        masks = _masks(name)
        kinds = sorted(k[len('scores_'):] for k in mfma if k.startswith('scores_'))
        ref = {}
        for k in kinds:
            assert np.array_equal(valu[f'X_{k}'], mfma[f'X_{k}']), k
            ref[k] = orc.doppler_scores(mfma[f'X_{k}'], masks, mfma['shifts'], True)
        _runs[name] = (valu, mfma, ref, masks)
    return _runs[name]


def _per_bin_err(got, ref):
    """error of every bin at or above 1e-4 of the block's largest score, relative to that bin's own score"""
    g, s = got[:, 0].astype(np.float64), ref[:, 0]
    keep = s >= 1e-4 * s.max()
    return np.abs(g[keep] - s[keep]) / s[keep]


def _unique_counts(masks):
    """how often each unique filter counts: exact copies and exact negatives count with the first of their kind"""
    n = []
    seen = []
    for m in masks:
        for i, u in enumerate(seen):
            if np.array_equal(m, u) or np.array_equal(m, -u):
                n[i] += 1
                break
        else:
            seen.append(m)
            n.append(1)
    return n


@pytest.mark.parametrize('name', ['bench_FSK', 'bench_GFSK'])
def test_shipped_banks_against_the_oracle_on_adversarial_blocks(name, tmp_path_factory):
    """bench_FSK and bench_GFSK (8 unique filters of 48 taps at 16 samples per symbol: the matrix form) on wrap_child.py's inputs, with
    the tolerances of test_wrap_mfma_against_the_oracle_on_adversarial_blocks: per bin within 1e-5 of the oracle and no more than
    twice as far from it as the vector form plus 2e-7."""
    valu, mfma, ref, masks = _bank_run(name, tmp_path_factory)
    _, T, _ = filter_support(masks)
    counts = _unique_counts(masks)
    assert (len(counts), T) == (8, 48) and int(mfma['taps']) == T and int(mfma['rows']) == len(counts)
    assert int(mfma['filter_side']) == 1 and int(mfma['log2L']) == 8
    assert wrap_form(N, counts, T, True) == 'matrix'
    worst, clear = {}, {}
    for k, r in ref.items():
        em, ev = _per_bin_err(mfma[f'scores_{k}'], r), _per_bin_err(valu[f'scores_{k}'], r)
        worst[k] = (float(em.max()), float(ev.max()))
        top = np.sort(r[:, 0])[::-1]
        clear[k] = top[0] - top[1] > 1e-4 * top[0] and top[1] - top[2] > 1e-4 * top[1]      # (see test_gpu_wrap_mfma.py)
    print(f'{name}: per-bin relative error (matrix cores, vector ALUs):', worst)
    for k in ref:
        assert not np.array_equal(mfma[f'scores_{k}'], valu[f'scores_{k}']), k            # the matrix form ran
        assert np.all(mfma[f'scores_{k}'][:, 1:] == 0), k
        if clear[k]:
            assert abs(float(mfma[f'pick_{k}'][0]) - float(valu[f'pick_{k}'][0])) < 1e-3, k
    for k, (em, ev) in worst.items():
        assert em <= 1e-5, (k, em, ev)
        assert em <= 2 * ev + 2e-7, (k, em, ev)


@pytest.mark.parametrize('name,rank', [('bench_GMSK', 6), ('bench_FSK', 4)])
def test_span_basis_on_the_matrix_form(name, rank, tmp_path_factory):
    """``set_search_basis('span')`` at 2^18 samples: fewer rows than the tile has columns.  Against the oracle's FULL bank within 1e-5,
    against the default basis of the same handle within 2e-6 (the figures of test_span_basis_search_equals_full_bank), columns 1...
    zero; and the matrix form is the one that ran."""
    valu, mfma, ref, masks = _bank_run(name, tmp_path_factory)
    _, T, _ = filter_support(masks)
    assert int(mfma['span_rows']) == rank and int(mfma['span_filter_side']) == 1
    assert wrap_form(N, _unique_counts(masks), T, True, span_rank=rank) == 'matrix'
    worst = 0.0
    for k, r in ref.items():
        for form, res in (('vector', valu), ('matrix', mfma)):
            sp, full = res[f'spanscores_{k}'].astype(np.float64), res[f'scores_{k}'].astype(np.float64)
            e_ref, e_full = np.abs(sp - r).max() / r.max(), np.abs(sp - full).max() / full.max()
            worst = max(worst, e_ref)
            assert e_ref < 1e-5, (k, form, e_ref)
            assert e_full < 2e-6, (k, form, e_full)
            assert np.all(sp[:, 1:] == 0), (k, form)
            oidx, _ = orc.find_doppler_est(res[f'spanscores_{k}'], len(sp), 0, True)
            assert _same(res[f'spanpick_{k}'][0], oidx), (k, form)
        assert not np.array_equal(mfma[f'spanscores_{k}'], valu[f'spanscores_{k}']), k
    print(f'{name}, span basis ({rank} rows): worst error relative to the largest score {worst:.2e}')


# ---- 3. ... 5. the call paths ----------------------------------------------------------------------------------------------------------
def _calls(tmp_path, mode, form):
    out = str(tmp_path / f'{mode}{form}.npz')
    subprocess.run([sys.executable, CALLS, mode, out], check=True, env=_env(form), timeout=600)
    return dict(np.load(out))


def test_batches_equal_single_blocks_bit_for_bit(tmp_path):
    """begin_blocks with 5 and with 3 blocks of 2^18 samples from a window (k_segw with nblk > 1) against the same blocks one per call
    on a second handle: scores and picks bit for bit, default and span basis, one block all zeros (NaN index) -- in both forms, and
    the two forms' tables differ: the matrix form is the one in force."""
    valu, mfma = _calls(tmp_path, 'batches', '0'), _calls(tmp_path, 'batches', '1')
    assert int(mfma['rows_filters']) == 8 and int(mfma['rows_span']) == 6
    for basis in ('filters', 'span'):
        for form, r in (('vector', valu), ('matrix', mfma)):
            for nb in (5, 3):
                for b in range(nb):
                    tag = (basis, form, nb, b)
                    assert np.array_equal(r[f'batch{nb}_{basis}_scores{b}'], r[f'single_{basis}_scores{b}']), tag
                    assert _same(r[f'batch{nb}_{basis}_pick{b}'], r[f'single_{basis}_pick{b}']), tag
            for b in range(5):
                s, p = r[f'single_{basis}_scores{b}'], r[f'single_{basis}_pick{b}']
                if b == 1:
                    assert not s.any() and np.isnan(p[0]) and p[2] == 0, (basis, form)
                else:
                    assert s[:, 0].min() > 0 and not s[:, 1:].any() and np.isfinite(p[0]) and p[2] == 1, (basis, form, b)
        for b in (0, 2, 3, 4):
            assert not np.array_equal(mfma[f'batch5_{basis}_scores{b}'], valu[f'batch5_{basis}_scores{b}']), (basis, b)
            a, m = valu[f'batch5_{basis}_scores{b}'].astype(np.float64), mfma[f'batch5_{basis}_scores{b}'].astype(np.float64)
            assert np.abs(a - m).max() / a.max() < 2e-6, (basis, b)


def test_power_of_two_scaling_is_exact_on_the_device(tmp_path):
    """scores(2^k x) == 2^(2k) scores(x) bit for bit, with the same index picked: both scales of the split-fp16 product are powers of
    two taken from the data, and no threshold of the kernel depends on absolute amplitude.  (The pick's second number, the metric,
    is 10 log10 of a value that scales with the scores: not compared.)"""
    r = _calls(tmp_path, 'scaling', '1')
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    assert sorted(r['ks']) == [-30, -9, 1, 20]
    for name in ('stream', 'burst+0'):
        s0, p0 = r[f'{name}_k0_scores'], r[f'{name}_k0_pick']
        assert s0.dtype == np.float32 and s0[:, 0].min() > 0 and not s0[:, 1:].any()
        for k in (int(v) for v in r['ks']):
            sk, pk = r[f'{name}_k{k}_scores'], r[f'{name}_k{k}_pick']
            want = np.ldexp(s0.astype(np.float64), 2 * k)
            assert tiny <= want[:, 0].min() and want[:, 0].max() <= huge, (name, k)      # every score a normal float32
            assert np.array_equal(sk, want.astype(np.float32)) and np.array_equal(sk.astype(np.float64), want), (name, k)
            assert pk[0] == p0[0], (name, k, pk, p0)


def test_live_handles_equal_fresh_ones(tmp_path):
    """The per-bin tables are cached on (rows, span, segment length, K-steps): after set_shifts, after set_filters to a bank on the
    vector form (49 taps) and back, and after a basis switch and back, a live handle scores what a fresh handle scores, bit for bit."""
    r = _calls(tmp_path, 'live', '1')
    counts = [1] * 8
    assert int(r['taps_gmsk']) == 48 and int(r['taps_other']) == 49 and int(r['log2L_other']) == 8
    assert wrap_form(N, counts, 48, True) == 'matrix' and wrap_form(N, counts, 49, True) == 'vector'
    pairs = [('shifts_ab', 'shifts_b_fresh'), ('filters_other', 'filters_other_fresh'), ('filters_back', 'gmsk_fresh'),
             ('shifts_a', 'gmsk_fresh'), ('basis_filters', 'gmsk_fresh'), ('basis_span1', 'span_fresh'), ('basis_span2', 'span_fresh')]
    for live, fresh in pairs:
        assert np.array_equal(r[f'{live}_scores'], r[f'{fresh}_scores']), (live, fresh)
        assert _same(r[f'{live}_pick'], r[f'{fresh}_pick']), (live, fresh)
        assert r[f'{fresh}_scores'][:, 0].min() > 0
    # ... and the steps in between did change the tables
    for a, b in (('shifts_a', 'shifts_ab'), ('filters_other', 'filters_back'), ('basis_span1', 'basis_filters')):
        assert not np.array_equal(r[f'{a}_scores'], r[f'{b}_scores']), (a, b)
