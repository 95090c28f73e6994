"""The schedules of the bin loop of the matrix-core search (wrap_kernels.hpp, k_segw) that the other files leave out.  A step of the
loop issues one bin's products with the bin before's squares, reduction and row between them, and stores that row at the head of the
step after; the one-bin, one-slot rectangle never enters a step (products, then the finish, alone), so it is a second schedule of the
same arithmetic and the reference here, held to the oracle itself.  bench_GMSK at 2^18 samples, every rectangle in a child of its own
(tests/children/issue_child.py, MFB_SEG_FSM_RECT read once per process), one child at a time.
  D = 3,   3,1:    an odd count of bins, left at the first exit after one step
  D = 4,   4,2:    an even count, two slots a wave
  D = 129, 129,1 and D = 130, 130,1: more than 64 bins in a rectangle.  The planner leaves a set rectangle alone and groups the slots, so
                   a wave walks chunks of 64, 64 and 1 or 2 bins: the bins' powers of two are fetched again per chunk and waited for in
                   front of it, and the rows' buffer is rebased per chunk."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import mfbank_oracle as orc

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'issue_child.py')
NAME, LOG2N = 'bench_GMSK', 18
PARITY_TOL = 1e-5                       # of the table's largest score (bench.py's north star), as tests/test_gpu_wrap_binloop.py
KINDS = ('stream', 'zero_segment')
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')
# D -> (rectangle, whether the 1,1 table is held to the oracle)
CASES = {3: ('3,1', True), 4: ('4,2', False), 129: ('129,1', False), 130: ('130,1', True)}


def _child(tmp_path, D, rect, spectrum):
    out = str(tmp_path / f'd{D}_{rect.replace(",", "_")}.npz')
    env = dict({k: v for k, v in os.environ.items() if k not in DROP}, MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=rect)
    p = subprocess.run([sys.executable, CHILD, str(D), out] + (['spectrum'] if spectrum else []), env=env, timeout=300)
    assert p.returncode == 0, (D, rect, p.returncode)
    return dict(np.load(out))


@pytest.mark.gpu
@pytest.mark.parametrize('D', sorted(CASES))
def test_the_rectangle_scores_the_bits_of_the_one_bin_one_slot_rectangle(tmp_path, D):
    """The table is bit-equal to the 1,1 table and the pick equal, on both inputs; the rectangle asked for is the one that ran
    (mfb_get_search_info); at D = 3 and D = 130 the 1,1 table is within PARITY_TOL of the oracle."""
    rect, parity = CASES[D]
    ref = _child(tmp_path, D, '1,1', parity)
    assert int(ref['filter_side']) == 1 and int(ref['log2L']) == 8 and int(ref['bins_per_forward']) == 1, ref
    pool = want = None
    if parity:                          # the oracle of the reference tables, while the other child runs
        from pycusdr_amd import config as cfg
        from pycusdr_amd.protocol import loadProtocol
        conf = cfg.bench_config(NAME, blockSize=LOG2N, doppCarrierSteps=D)
        _, masks = loadProtocol(NAME)(conf=conf).get_filter(1 << LOG2N, 16, 3)
        pool = ThreadPoolExecutor(len(KINDS))
        want = {k: pool.submit(orc.doppler_scores, ref[f'X_{k}'], masks, ref['shifts'], True) for k in KINDS}
        pool.shutdown(wait=False)
    r = _child(tmp_path, D, rect, False)
    assert int(r['filter_side']) == 1 and int(r['log2L']) == 8
    assert int(r['bins_per_forward']) == int(rect.split(',')[0]), (rect, int(r['bins_per_forward']))
    for k in KINDS:
        assert r[f'scores_{k}'].shape[0] == D
        assert np.array_equal(r[f'scores_{k}'], ref[f'scores_{k}']), (rect, k)
        assert np.array_equal(r[f'pick_{k}'], ref[f'pick_{k}'], equal_nan=True), (rect, k)
    if parity:
        for k in KINDS:
            w = want[k].result()
            rel = np.abs(ref[f'scores_{k}'][:, 0].astype(np.float64) - w[:, 0]).max() / w[:, 0].max()     # (column 0: the sum)
            print(f'D = {D}, {k}: 1,1 table against the oracle {rel:.3e}')
            assert rel < PARITY_TOL, (k, rel)
