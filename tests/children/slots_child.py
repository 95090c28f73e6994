"""Child of tests/test_gpu_wrap_slots.py: the doppSum tables and picks of the matrix-core search (wrap_kernels.hpp, k_segw) in THIS
process's rectangle (MFB_SEG_FSM_RECT in the environment, or the planner's default without it: read once per process), with the
bench_GMSK bank at 2^18 samples.  Asserts that the search ran on the filter side with 256-point segments; writes an .npz.
usage: slots_child.py tables <D> <out.npz>     the two inputs of binloop_child.py on a handle of D bins
       slots_child.py batch <D> <out.npz>      two blocks of a window as one batch, and the same two blocks one per call"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binloop_child import NAME, inputs                                                 # noqa: E402
from wrap_child import cfg, loadProtocol, setup, sg                                    # noqa: E402
from pycusdr_amd.demodulator import UHF, Operations                                    # noqa: E402

LOG2N = 18
N = 1 << LOG2N


def _form(bank):
    info, path = bank.get_search_info(), bank.get_search_path()
    assert int(info['filter_side']) == 1 and path['log2L'] == 8, (info, path)
    return {'filter_side': int(info['filter_side']), 'log2L': path['log2L'], 'bins_per_forward': int(info['bins_per_forward'])}


def tables(D, res):
    bank, _, _ = setup(NAME, LOG2N, D)
    try:
        res.update(_form(bank))
        for k, x in inputs(N, bank.get_search_path()['valid_per_segment']).items():
            bank.upload(x)
            res[f'pick_{k}'] = np.asarray(bank.find_carrier(), dtype=np.float64)
            res[f'scores_{k}'] = bank.get_scores()
    finally:
        bank.close()


def batch(D, res):
    ov, nb = 1 << 10, 2
    step = N - ov
    conf = cfg.bench_config(NAME, blockSize=LOG2N, doppCarrierSteps=D)
    sig = sg.s1_stream(nb, N, ov, 'GMSK', snr_db=9.0, seed=23)[:nb * step + ov].astype(np.complex64)
    bat, one = (UHF.Demodulator(conf, loadProtocol(NAME)(conf=conf), 'UHF-H') for _ in range(2))
    K = dict(k_offset=bat.codeRateAndPhaseOffsetHigh, k_len=bat.codeRateAndPhaseOffsetLow - bat.codeRateAndPhaseOffsetHigh,
             spsym_min=bat.spsymMin, op=Operations.CENTRES_ABS.value)
    try:
        res.update(_form(bat.bank))
        _form(one.bank)
        bat.bank.windows(nb, step)[0][:] = sig
        bat.bank.begin_blocks(0, nb, **K)
        blocks = bat.bank.end_blocks(0)
        assert len(blocks) == nb
        for b, r in enumerate(blocks):
            res[f'batch_scores{b}'] = bat.bank.get_batch_scores(b)
            res[f'batch_pick{b}'] = np.array([r['pick'][0], r['pick'][1], float(r['pick_valid'])], dtype=np.float64)
            one.bank.input[:] = sig[b * step:b * step + N]
            r = one.bank.receive_block(**K)
            res[f'single_scores{b}'] = one.bank.get_scores()
            res[f'single_pick{b}'] = np.array([r['pick'][0], r['pick'][1], float(r['pick_valid'])], dtype=np.float64)
    finally:
        bat.close()
        one.close()


if __name__ == '__main__':
    out = {}
    {'tables': tables, 'batch': batch}[sys.argv[1]](int(sys.argv[2]), out)
    np.savez(sys.argv[3], **out)
