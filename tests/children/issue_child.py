"""Child of tests/test_gpu_wrap_issue.py: the doppSum tables and picks of the two blocks of binloop_child.py from a handle of D bins, in
THIS process's rectangle of the matrix-core search (MFB_SEG_FSM_RECT in the environment is read once per process), with the bins per
forward transform that mfb_get_search_info reports; with ``spectrum`` also the blocks' spectra and the shifts (for the oracle).
usage: issue_child.py <D> <out.npz> [spectrum]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binloop_child import NAME, inputs                                                 # noqa: E402
from wrap_child import setup                                                           # noqa: E402

LOG2N = 18


def main(D, out, spectrum=False):
    bank, _, shifts = setup(NAME, LOG2N, D)
    try:
        info, path = bank.get_search_info(), bank.get_search_path()
        res = {'filter_side': int(info['filter_side']), 'log2L': path['log2L'], 'bins_per_forward': int(info['bins_per_forward'])}
        if spectrum:
            res['shifts'] = np.asarray(shifts)
        for k, x in inputs(1 << LOG2N, path['valid_per_segment']).items():
            bank.upload(x)
            res[f'pick_{k}'] = np.asarray(bank.find_carrier(), dtype=np.float64)
            res[f'scores_{k}'] = bank.get_scores()
            if spectrum:
                res[f'X_{k}'] = bank.get_spectrum()
        np.savez(out, **res)
    finally:
        bank.close()


if __name__ == '__main__':
    main(int(sys.argv[1]), sys.argv[2], spectrum=len(sys.argv) > 3 and sys.argv[3] == 'spectrum')
