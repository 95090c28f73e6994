"""Randomised sweep of the 256-point search at the block lengths where the wrap-around energy runs on the matrix cores (2^18 samples
and more; wrap_kernels.hpp, k_segw), in both forms, against the fp64 oracle: random bins over the whole of [0, N), a noise bin,
synthetic banks of 1 ... 16 unique filters (rank-deficient, with an exact negative, every filter twice), 30 ... 52 taps with the edges
of the matrix form's range (33 | 34 and 48 | 49) in the first cases, the support window anywhere in the block (wrapping around its end
too), banks and inputs scaled over many decades, a segment 10^4 above the rest, single full-scale samples on a floor, the span basis.

MFB_SEG_WRAP_MFMA is read once per process, so each form runs in a child of its own (``--child``) and writes its score tables to an
.npz; the parent runs the oracle and the checks (tests/test_gpu_wrap_sweep.py calls the same functions).
usage: python tests/tools/fuzz_wrap.py [cases] [seed]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from seg_model import wrap_form                                                       # noqa: E402

# the seed: the first from 1 upward with which -- by ``expected`` alone, no device -- at least half of the cases take the matrix form,
# a bank of 16 unique filters and one with an exact negative run the vector form with the default basis and the matrix form with the
# span basis, the matrix form runs with 8 rows, and three or more support windows wrap around the end of the block
# (tests/test_wrap_model.py holds the draw to that)
CASES, SEED = 25, 4
EDGE_TAPS = (33, 34, 48, 49)          # 33 | 34: 14 | 13 valid register slots; 48 | 49: the tap bound of the instantiated K-steps
NOISE_KINDS = ('noise', 'scaled')


def draw(cases=CASES, seed=SEED):
    """The cases' parameters (plain numbers; ``build`` makes the arrays from ``sub``)."""
    rs = np.random.RandomState(seed)
    out = []
    for case in range(cases):
        edge, big_d, big_n = case < len(EDGE_TAPS), case == len(EDGE_TAPS), case == len(EDGE_TAPS) + 1
        log2N = 20 if big_n else int(rs.randint(18, 20))
        sum_all = True if edge else bool(rs.randint(0, 4))
        doff = int(rs.randint(0, 2))
        # (the edge cases keep everything else inside the matrix form's range, so that the tap count alone decides; the case with
        # hundreds of bins and the 2^20 case keep the oracle's cost down with few filters)
        M = int(rs.choice([1, 2, 3] if big_d else [2, 3, 5, 8] if big_n or edge else [1, 2, 3, 5, 8, 16]))
        rank = int(rs.randint(1, min(M, 8) + 1))
        T = EDGE_TAPS[case] if edge else int(rs.randint(30, 53))
        dup = ['none', 'none', 'neg', 'twice'][rs.randint(0, 4)]
        if dup == 'neg' and (M < 3 or edge):
            dup = 'none'
        if dup == 'twice' and big_n:
            dup = 'none'
        if dup == 'neg':
            rank = min(rank, M - 1)                                  # filter 2 becomes minus filter 0
        Mtot = 2 * M if dup == 'twice' else M
        D = int(rs.randint(200, 400)) if big_d else int(rs.randint(1, 41))
        D = max(1, min(D, (1600 if big_d else 768) // (Mtot << (log2N - 18))))     # the oracle: ~0.1 s per 8 (bin, filter) transforms of 2^18 points
        kind = ['noise', 'noise', 'scaled', 'scaled', 'segment', 'spikes'][rs.randint(0, 6)]
        # the support window anywhere in the block; in one case of four its taps wrap around the block's end
        start = (1 << log2N) - int(rs.randint(1, T)) if rs.randint(0, 4) == 0 else int(rs.randint(0, 1 << log2N))
        out.append(dict(case=case, log2N=log2N, D=D, doff=doff, M=M, Mtot=Mtot, rank=rank, T=T, start=start,
                        dup=dup, bank_scale=float(10 ** rs.uniform(-6, 2)), sum_all=sum_all, kind=kind,
                        in_scale=float(10 ** rs.uniform(-12, 12)) if kind == 'scaled' else 1.0, sub=int(rs.randint(0, 2 ** 31 - 1))))
    return out


def counts(c):
    """how often each unique filter of case c's bank counts"""
    n = [2 if c['dup'] == 'twice' else 1] * c['M']
    if c['dup'] == 'neg':
        n[0] += 1
        del n[2]
    return n


def expected(c, basis):
    N = 1 << c['log2N']
    return wrap_form(N, counts(c), c['T'], c['sum_all'], span_rank=c['rank'] if basis == 'span' else None)


def bases(c):
    return ('filters', 'span') if c['sum_all'] else ('filters',)


def build(c):
    """masks complex64 [Mtot][N], x complex64 [N], shifts int32 [D + doff] of case c"""
    rs = np.random.RandomState(c['sub'])
    N, M, T, rank = 1 << c['log2N'], c['M'], c['T'], c['rank']
    h = np.zeros((M, N), dtype=np.complex128)
    basis = rs.standard_normal((rank, T)) + 1j * rs.standard_normal((rank, T))
    mix = rs.standard_normal((M, rank)) + 1j * rs.standard_normal((M, rank))
    h[:, (c['start'] + np.arange(T)) % N] = c['bank_scale'] * (mix @ basis)
    masks = np.fft.fft(h, axis=1).astype(np.complex64)
    if c['dup'] == 'neg':
        masks[2] = -masks[0]                                # an exact negative, counted with filter 0: the rows no longer count equally
    if c['dup'] == 'twice':
        masks = np.concatenate([masks, masks])              # every filter twice: equal counts
    x = rs.standard_normal(N) + 1j * rs.standard_normal(N)
    if c['kind'] == 'scaled':
        x *= c['in_scale']
    elif c['kind'] == 'segment':
        p = int(rs.randint(0, N - 256))
        x[p:p + 256] *= 1e4
    elif c['kind'] == 'spikes':
        x *= 1e-4
        pos = rs.randint(0, N, int(rs.randint(1, 7)))
        x[pos] = np.exp(2j * np.pi * rs.random_sample(len(pos)))
    shifts = rs.randint(0, N, c['D'] + c['doff']).astype(np.int32)
    return masks, x.astype(np.complex64), shifts


def child(out, cases, seed):
    """this process's form of the search on every case: tables, picks, the device's spectrum and what it made of the bank"""
    from pycusdr_amd.mfbank import MFBank
    res = {}
    for c in draw(cases, seed):
        masks, x, shifts = build(c)
        bank = MFBank(c['log2N'], c['D'], c['Mtot'], sum_all_masks=c['sum_all'], doppler_offset=c['doff'])
        try:
            bank.set_filters(masks)
            bank.set_shifts(shifts)
            bank.set_search_path('segment', 8)              # the segment length fixed: the case tests the form, not the chooser
            bank.upload(x)
            k = c['case']
            res[f'X{k}'] = bank.get_spectrum()
            for basis in bases(c):
                bank.set_search_basis(basis)
                res[f'pick{k}_{basis}'] = np.asarray(bank.find_carrier(), dtype=np.float64)
                res[f'scores{k}_{basis}'] = bank.get_scores()
                path, info = bank.get_search_path(), bank.get_search_info()
                res[f'meta{k}_{basis}'] = np.array([path['log2L'], path['taps'], bank.get_search_basis()[1], int(info['filter_side'])])
        finally:
            bank.close()
    np.savez(out, **res)


def run_form(form, out, cases=CASES, seed=SEED, timeout=900):
    env = dict(os.environ, MFB_SEG_WRAP_MFMA=form)
    for k in ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP'):
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out, str(cases), str(seed)], check=True, env=env, timeout=timeout)
    return dict(np.load(out))


def per_bin_err(got, ref):
    """error of every bin relative to that bin's own score (SUM_ALL tables: column 0); no bin may be too small to count"""
    g, s = got[:, 0].astype(np.float64), ref[:, 0]
    assert np.all(s >= 1e-4 * s.max()), 'a bin below 1e-4 of the largest'
    return np.abs(g - s) / s


def check(valu, mfma, cases=CASES, seed=SEED, log=print):
    """Every table of both forms against the oracle, which form ran against ``expected``.  Returns a summary dict; raises
    AssertionError with the case's parameters on the first miss."""
    from oracle import mfbank_oracle as orc
    worst = {'matrix': 0.0, 'vector': 0.0}
    worst_bin = {'matrix': 0.0, 'vector': 0.0}
    took = dict(cases=0, filters=0, span=0)
    for c in draw(cases, seed):
        k = c['case']
        masks, _, shifts = build(c)
        assert np.array_equal(valu[f'X{k}'], mfma[f'X{k}']), c
        ref = orc.doppler_scores(mfma[f'X{k}'], masks, shifts, c['sum_all'])
        assert 1e-30 < ref.max() < 1e36, ('the scores leave the range of float32', c)
        matrix_runs = 0
        for basis in bases(c):
            want = expected(c, basis)
            rows = len(counts(c)) if basis == 'filters' else c['rank']
            for name, r in (('vector', valu), ('matrix', mfma)):
                ds, pick, meta = r[f'scores{k}_{basis}'], r[f'pick{k}_{basis}'], r[f'meta{k}_{basis}']
                tag = dict(c, basis=basis, process=name, expected=want)
                assert list(meta) == [8, c['T'], rows, 1], (tag, list(meta))     # 256 points, the drawn support, the rows transformed
                err = float(np.abs(ds - ref).max() / ref.max())
                oidx, _ = orc.find_doppler_est(ds, c['D'], c['doff'], c['sum_all'])
                assert err < 1e-5, (tag, err)
                assert pick[0] == oidx or (np.isnan(pick[0]) and np.isnan(oidx)), (tag, float(pick[0]), float(oidx))
                form = want if name == 'matrix' else 'vector'
                worst[form] = max(worst[form], err)
            s0, s1 = valu[f'scores{k}_{basis}'], mfma[f'scores{k}_{basis}']
            tag = dict(c, basis=basis, expected=want)
            if want == 'matrix':
                assert not np.array_equal(s0, s1), ('the matrix form did not run', tag)
                matrix_runs += 1
                took[basis] += 1
                if c['kind'] in NOISE_KINDS:
                    em, ev = float(per_bin_err(s1, ref).max()), float(per_bin_err(s0, ref).max())
                    worst_bin['matrix'], worst_bin['vector'] = max(worst_bin['matrix'], em), max(worst_bin['vector'], ev)
                    assert em <= 2 * ev + 2e-7, (tag, em, ev)
            else:
                assert np.array_equal(s0, s1), ('the two settings differ where the vector form runs in both', tag)
        took['cases'] += 1 if matrix_runs else 0
        log(f"case {k}: 2^{c['log2N']} x {c['D']}+{c['doff']} bins, {c['Mtot']} filters ({len(counts(c))} unique, rank {c['rank']}, "
            f"{c['dup']}), {c['T']} taps at {c['start']}, sum_all {c['sum_all']}, {c['kind']}: "
            + ', '.join(f'{b} -> {expected(c, b)}' for b in bases(c)))
    return dict(cases=cases, seed=seed, matrix_cases=took['cases'], matrix_filters=took['filters'], matrix_span=took['span'],
                worst=worst, worst_bin=worst_bin)


def summary_line(s):
    return (f"{s['cases']} random cases ok (seed {s['seed']}): {s['matrix_cases']} took the matrix form ({s['matrix_filters']} with the "
            f"default basis, {s['matrix_span']} with the span basis); worst error relative to the table's largest score: matrix form "
            f"{s['worst']['matrix']:.2e}, vector form {s['worst']['vector']:.2e}; worst per-bin error on noise: matrix form "
            f"{s['worst_bin']['matrix']:.2e}, vector form {s['worst_bin']['vector']:.2e}")


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else CASES
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else SEED
    with tempfile.TemporaryDirectory() as d:
        valu = run_form('0', os.path.join(d, 'wrap0.npz'), cases, seed)
        mfma = run_form('1', os.path.join(d, 'wrap1.npz'), cases, seed)
    try:
        s = check(valu, mfma, cases, seed)
    except AssertionError as e:
        print('FAIL', e)
        sys.exit(1)
    print(summary_line(s))
    sys.exit(0 if 2 * s['matrix_cases'] >= cases else 1)
