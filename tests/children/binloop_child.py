"""Child of tests/test_gpu_wrap_binloop.py: the doppSum tables and picks of two blocks from a handle of D bins, in THIS process's
rectangle and form of the 256-point search (MFB_SEG_FSM_RECT and MFB_SEG_WRAP_MFMA in the environment are read once per process).
Writes an .npz with, per input, the scores and the pick; with ``spectrum`` also the block's spectrum (for the oracle).
usage: binloop_child.py <log2N> <D> <out.npz> [spectrum]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wrap_child import setup, sg                                                      # noqa: E402

NAME = 'bench_GMSK'


def inputs(N, V):
    """name -> complex64 block: the seeded S1 stream, and noise with one segment of 256 samples all zero (the split of that segment
    sees a largest component of 0 and the exponent 0)."""
    rs = np.random.RandomState(11)
    out = {'stream': sg.s1_stream(1, N, 1 << 10, 'GMSK', snr_db=8.0, seed=41)[:N]}
    x = (rs.standard_normal(N) + 1j * rs.standard_normal(N)) / np.sqrt(2)
    x[37 * V:37 * V + 256] = 0
    out['zero_segment'] = x
    return {k: np.asarray(v, dtype=np.complex64) for k, v in out.items()}


def main(log2N, D, out, spectrum=False):
    bank, _, shifts = setup(NAME, log2N, D)
    path = bank.get_search_path()
    res = {'shifts': np.asarray(shifts), 'filter_side': int(bank.get_search_info()['filter_side']), 'log2L': path['log2L']}
    for k, x in inputs(1 << log2N, path['valid_per_segment']).items():
        bank.upload(x)
        res[f'pick_{k}'] = np.asarray(bank.find_carrier(), dtype=np.float64)
        res[f'scores_{k}'] = bank.get_scores()
        if spectrum:
            res[f'X_{k}'] = bank.get_spectrum()
    np.savez(out, **res)
    bank.close()


if __name__ == '__main__':
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], spectrum=len(sys.argv) > 4 and sys.argv[4] == 'spectrum')
