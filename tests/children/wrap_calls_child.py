"""Child of tests/test_gpu_wrap_sweep.py: the call paths that reach the 256-point search at 2^18 samples, in THIS process's form of it
(MFB_SEG_WRAP_MFMA in the environment is read once per process), with the bench_GMSK bank.  Writes an .npz of score tables and picks;
the parent compares them.
usage: wrap_calls_child.py batches|scaling|live <out.npz>

batches   five blocks from a window (block stride N - 2^10, block 1 all zeros) as one batch of 5 and one of 3 on one handle, and one
          block per call on a second handle; default and span basis
scaling   the stream and burst+0 inputs of wrap_child.py times 2^k
live      set_shifts, set_filters and set_search_basis on a live handle against fresh handles"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pycusdr_amd import config as cfg, signals as sg                                  # noqa: E402
from pycusdr_amd.demodulator import UHF, Operations                                    # noqa: E402
from pycusdr_amd.mfbank import MFBank                                                  # noqa: E402
from pycusdr_amd.protocol import loadProtocol                                          # noqa: E402
from wrap_child import inputs, setup                                                   # noqa: E402

LOG2N = 18
N = 1 << LOG2N
SCALING_K = (-30, -9, 1, 20)


def _search(bank, x):
    bank.upload(x)
    pick = bank.find_carrier()
    return bank.get_scores(), np.asarray(pick, dtype=np.float64)


def batches(res):
    D, ov, nblocks = 48, 1 << 10, 5
    step = N - ov
    conf = cfg.bench_config('bench_GMSK', blockSize=LOG2N, doppCarrierSteps=D)
    sig = sg.s1_stream(nblocks, N, ov, 'GMSK', snr_db=9.0, seed=11)[:nblocks * step + ov].astype(np.complex64)
    sig[step:step + N] = 0                          # block 1 is all zeros: a NaN index
    bat, one = (UHF.Demodulator(conf, loadProtocol('bench_GMSK')(conf=conf), 'UHF-H') for _ in range(2))
    K = dict(k_offset=bat.codeRateAndPhaseOffsetHigh, k_len=bat.codeRateAndPhaseOffsetLow - bat.codeRateAndPhaseOffsetHigh,
             spsym_min=bat.spsymMin, op=Operations.CENTRES_ABS.value)
    try:
        for basis in ('filters', 'span'):
            for d in (bat, one):
                d.bank.set_search_basis(basis)
                assert d.bank.get_search_basis()[0] == basis and d.bank.get_search_path()['log2L'] == 8
            res[f'rows_{basis}'] = bat.bank.get_search_basis()[1]
            for nb in (5, 3):
                win = bat.bank.windows(nb, step)[0]
                win[:] = sig[:nb * step + ov]
                bat.bank.begin_blocks(0, nb, **K)
                blocks = bat.bank.end_blocks(0)
                assert len(blocks) == nb
                for b, r in enumerate(blocks):
                    res[f'batch{nb}_{basis}_scores{b}'] = bat.bank.get_batch_scores(b)
                    res[f'batch{nb}_{basis}_pick{b}'] = np.array([r['pick'][0], r['pick'][1], float(r['pick_valid'])], dtype=np.float64)
            for b in range(nblocks):
                one.bank.input[:] = sig[b * step:b * step + N]
                r = one.bank.receive_block(**K)
                res[f'single_{basis}_scores{b}'] = one.bank.get_scores()
                res[f'single_{basis}_pick{b}'] = np.array([r['pick'][0], r['pick'][1], float(r['pick_valid'])], dtype=np.float64)
    finally:
        bat.close()
        one.close()


def scaling(res):
    bank, _, shifts = setup('bench_GMSK', LOG2N, 32)
    res['ks'] = np.array(SCALING_K)
    try:
        V = bank.get_search_path()['valid_per_segment']
        xs = inputs(N, shifts, V)
        for name in ('stream', 'burst+0'):
            x = xs[name]
            for k in (0,) + SCALING_K:
                xk = (np.ldexp(x.real, k) + 1j * np.ldexp(x.imag, k)).astype(np.complex64)
                assert np.array_equal(np.ldexp(xk.real, -k), x.real) and np.array_equal(np.ldexp(xk.imag, -k), x.imag)    # exact
                res[f'{name}_k{k}_scores'], res[f'{name}_k{k}_pick'] = _search(bank, xk)
    finally:
        bank.close()


def synthetic_bank(M, T, seed=5):
    """M filters of T complex normal taps at the start of the block, as masks complex64 [M][N]"""
    rs = np.random.RandomState(seed)
    h = np.zeros((M, N), dtype=np.complex128)
    h[:, :T] = rs.standard_normal((M, T)) + 1j * rs.standard_normal((M, T))
    return np.fft.fft(h, axis=1).astype(np.complex64)


def live(res):
    D = 48
    bank, gmsk, a = setup('bench_GMSK', LOG2N, D)
    M = gmsk.shape[0]
    x = inputs(N, a, bank.get_search_path()['valid_per_segment'])['stream']
    b = ((np.asarray(a, dtype=np.int64) * 3 + 12345) % N).astype(np.int32)       # another table: other bins, other spacing
    other = synthetic_bank(M, 49)                                                # 49 taps: the vector form

    def fresh(masks, shifts, basis='filters'):
        f = MFBank(LOG2N, D, M)
        try:
            f.set_filters(masks)
            f.set_shifts(shifts)
            f.set_search_basis(basis)
            return _search(f, x)
        finally:
            f.close()
    try:
        res['shifts_a_scores'], res['shifts_a_pick'] = _search(bank, x)
        bank.set_shifts(b)
        res['shifts_ab_scores'], res['shifts_ab_pick'] = _search(bank, x)
        res['shifts_b_fresh_scores'], res['shifts_b_fresh_pick'] = fresh(gmsk, b)
        bank.set_shifts(a)
        res['taps_gmsk'] = bank.get_search_path()['taps']
        bank.set_filters(other)
        res['taps_other'], res['log2L_other'] = bank.get_search_path()['taps'], bank.get_search_path()['log2L']
        res['filters_other_scores'], res['filters_other_pick'] = _search(bank, x)
        res['filters_other_fresh_scores'], res['filters_other_fresh_pick'] = fresh(other, a)
        bank.set_filters(gmsk)
        res['filters_back_scores'], res['filters_back_pick'] = _search(bank, x)
        res['gmsk_fresh_scores'], res['gmsk_fresh_pick'] = fresh(gmsk, a)
        for step in ('span1', 'filters', 'span2'):
            bank.set_search_basis('filters' if step == 'filters' else 'span')
            res[f'basis_{step}_scores'], res[f'basis_{step}_pick'] = _search(bank, x)
        res['span_fresh_scores'], res['span_fresh_pick'] = fresh(gmsk, a, 'span')
    finally:
        bank.close()


if __name__ == '__main__':
    out = {}
    {'batches': batches, 'scaling': scaling, 'live': live}[sys.argv[1]](out)
    np.savez(sys.argv[2], **out)
