"""The bin loop of the matrix-core search (wrap_kernels.hpp, k_segw): bin jb's squares, reduction and store issue under bin jb + 1's
products, from two sets of accumulators and bin tables taking turns, and the bins' powers of two are fetched once per rectangle.
Whatever a wave carries from bin to bin or slot to slot must not reach the bits: every rectangle (MFB_SEG_FSM_RECT = bins,slots)
is held to the one-bin, one-slot rectangle, which carries nothing, and that one to the oracle.  The rectangle and the form are
read once per process: every (bins, rectangle) runs in a child of its own (tests/children/binloop_child.py)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import mfbank_oracle as orc

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'binloop_child.py')
NAME, LOG2N = 'bench_GMSK', 18          # the smallest block on the matrix-core form
PARITY_TOL = 1e-5                       # of the table's largest score (bench.py's north star)
# 1,1: no state from bin to bin or slot to slot, the reference of the others.  2,1 / 3,1: the unrolled pair alone and with a tail;
# 16,1: the default; 16,3 and 32,2: the last bin of a slot is flushed before the next slot rebuilds the fragments
RECTS = ('1,1', '2,1', '3,1', '16,1', '16,3', '32,2')
KINDS = ('stream', 'zero_segment')


def _children(tmp_path, D, masks):
    """{rectangle: tables of the matrix-core form}, and the vector form's (default rectangle); the children run side by side"""
    base = {k: v for k, v in os.environ.items() if k not in ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')}
    procs = {}
    for rect in RECTS + ('valu',):
        out = str(tmp_path / f'd{D}_{rect.replace(",", "_")}.npz')
        env = dict(base, MFB_SEG_WRAP_MFMA='0') if rect == 'valu' else dict(base, MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=rect)
        cmd = [sys.executable, CHILD, str(LOG2N), str(D), out] + (['spectrum'] if rect == '1,1' else [])
        procs[rect] = (subprocess.Popen(cmd, env=env), out)
    res = {}
    try:
        for rect, (p, out) in procs.items():
            assert p.wait(timeout=300) == 0, (D, rect)
            res[rect] = dict(np.load(out))
            if rect == '1,1':           # the oracle of the reference tables, while the other children run
                pool = ThreadPoolExecutor(len(KINDS))
                res['oracle'] = {k: pool.submit(orc.doppler_scores, res[rect][f'X_{k}'], masks, res[rect]['shifts'], True) for k in KINDS}
                pool.shutdown(wait=False)
    finally:
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('D', [1, 2, 17, 33])
def test_every_rectangle_scores_the_bits_of_the_one_bin_rectangle(tmp_path, D):
    """D = 1: a loop of one bin; 2: one unrolled pair; 17: a last chunk of one bin behind a full rectangle; 33: bins grouped by XCD
    with uneven shares.  Every table is bit-equal to the 1,1 table and every pick equal; the 1,1 table is within PARITY_TOL of the
    oracle; every run took the filter-side search on 256-point segments and its tables differ from the vector form's run, so the
    matrix-core form is what ran."""
    from pycusdr_amd import config as cfg
    from pycusdr_amd.protocol import loadProtocol
    conf = cfg.bench_config(NAME, blockSize=LOG2N, doppCarrierSteps=D)
    _, masks = loadProtocol(NAME)(conf=conf).get_filter(1 << LOG2N, 16, 3)
    res = _children(tmp_path, D, masks)
    ref, valu = res['1,1'], res['valu']
    for k in KINDS:
        want = res['oracle'][k].result()
        assert ref[f'scores_{k}'].shape[0] == D
        rel = np.abs(ref[f'scores_{k}'][:, 0].astype(np.float64) - want[:, 0]).max() / want[:, 0].max()     # (column 0: the sum)
        print(f'D = {D}, {k}: 1,1 table against the oracle {rel:.3e}')
        assert rel < PARITY_TOL, (k, rel)
    for rect in RECTS:
        r = res[rect]
        assert int(r['filter_side']) == 1 and int(r['log2L']) == 8, rect
        # the form is read once per process: what the run scored (both inputs) against the vector form's run.  (With one bin an
        # input's table is a single fp32 number, and the two forms, 1e-7 apart, can round to the same one: D = 1, stream.)
        assert any(not np.array_equal(r[f'scores_{k}'], valu[f'scores_{k}']) for k in KINDS), rect
        for k in KINDS:
            assert np.array_equal(r[f'scores_{k}'], ref[f'scores_{k}']), (rect, k)
            assert np.array_equal(r[f'pick_{k}'], ref[f'pick_{k}'], equal_nan=True), (rect, k)
