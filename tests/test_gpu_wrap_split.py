"""The split of the segment windows in the matrix-core search (wrap_kernels.hpp, k_segw): every window sample is scaled and split into
hi / lo fp16 once, by the lane that holds it, and the 160 fragment registers of a wave are reads of those words.  The fragments must
come out as they always did, so the tables must: bit for bit the tables that the library scored before the change
(tests/golden/segw_tables.npz; tests/golden/make_golden_segw.py says which commit wrote them and regenerates the inputs), and within
1e-5 of the fp64 oracle relative to the table's largest score (the bound of the other k_segw tests).

2^18 samples, the smallest block on this form.  Banks: bench_GMSK (48 taps) and 8 seeded filters of 34 taps (window slots below offset
-33 zeroed).  Handles: D = 2 and 33 on forced one-bin rectangles, D = 130 on forced 64,1 rectangles (chunks of 64, 64 and 2 bins); a
handle of D bins takes the first D shifts of one table, so one oracle table per (bank, block) serves all three.  Blocks
(tests/children/split_child.py): the seeded S1 stream; zeros with one full-scale segment (scale exponent 0 beside a scaled segment in
one wave); amplitudes stepping 2^0 ... 2^-20 from segment to segment (four scales in a slot); a full-scale burst on exactly one
segment's wrap window.  The oracle's tables are recorded in the fixture (four minutes of fp64 transforms); the test recomputes the two
bins of the D = 2 handle and holds the record to them.  One child per handle, under a timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mfbank_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'children'))
import split_child as sc                                                               # noqa: E402

CHILD = os.path.join(HERE, 'children', 'split_child.py')
GOLDEN = os.path.join(HERE, 'golden', 'segw_tables.npz')
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')
CASES = [(bank, D, rect) for bank in sc.BANKS for D, rect in ((2, '1,1'), (33, '1,1'), (130, '64,1'))]

_golden = {}


def golden():
    if not _golden:
        _golden.update(np.load(GOLDEN))
    return _golden


def _child(tmp_path, bank, D, rect):
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    env.update(MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=rect)
    out = str(tmp_path / f'{bank}_{D}.npz')
    subprocess.run([sys.executable, CHILD, bank, str(D), out], check=True, env=env, timeout=300)
    return dict(np.load(out))


def test_the_fixture_records_what_the_child_regenerates():
    g = golden()
    assert int(g['log2N']) == sc.LOG2N and int(g['V']) == sc.V and int(g['dmax']) == sc.DMAX and int(g['segment']) == sc.SEG
    assert int(g['scale_k']) == sc.SCALE_K
    assert sorted(g['seeds'].tolist()) == sorted(f'{k}={v}' for k, v in sc.SEEDS.items())
    assert sorted(g['taps'].tolist()) == sorted(f'{k}={v}' for k, v in sc.BANKS.items())
    assert str(g['tables_commit'])
    for bank, D, _ in CASES:
        for k in sc.KINDS:
            t = g[f'table_{bank}_{D}_{k}']
            assert t.dtype == np.float32 and t.shape == (D,) and t.min() > 0
            assert g[f'oracle_{bank}_{k}'].shape == (sc.DMAX,)


@pytest.mark.parametrize('bank', list(sc.BANKS))
def test_the_recorded_oracle_is_the_oracle(bank):
    """oracle.doppler_scores on the first two shifts, recomputed here: the record of all 130 was made the same way"""
    g = golden()
    shifts, xs, m = sc.shifts_table()[:2], sc.inputs(), sc.masks(bank)
    for k in sc.KINDS:
        ref = orc.doppler_scores(np.fft.fft(xs[k].astype(np.complex128)), m, shifts, True)[:, 0]
        assert np.allclose(ref, g[f'oracle_{bank}_{k}'][:2], rtol=1e-12, atol=0), (bank, k)


@pytest.mark.gpu
@pytest.mark.parametrize('bank,D,rect', CASES)
def test_tables_equal_the_recorded_ones_and_the_oracle(tmp_path, bank, D, rect):
    g = golden()
    r = _child(tmp_path, bank, D, rect)
    assert int(r['taps']) == sc.BANKS[bank] and int(r['bins_per_forward']) == int(rect.split(',')[0])
    for k in sc.KINDS:
        s = r[f'scores_{k}']
        assert s.dtype == np.float32 and s.shape[0] == D and not s[:, 1:].any(), k
        ref = g[f'oracle_{bank}_{k}'][:D]
        rel = np.abs(s[:, 0].astype(np.float64) - ref).max() / ref.max()
        same = np.array_equal(s[:, 0], g[f'table_{bank}_{D}_{k}'])
        print(f'{bank} D = {D} {k}: against the oracle {rel:.2e}, equal to the recorded table: {same}')
        assert same, (bank, D, k)
        assert rel < 1e-5, (bank, D, k, rel)
    # table(x 2^7) = table(x) 2^14, element for element: both scales of the split are powers of two taken from the data
    s0, sk = r['scores_stream'], r['scores_stream_scaled']
    want = np.ldexp(s0.astype(np.float64), 2 * sc.SCALE_K)
    assert np.array_equal(sk.astype(np.float64), want) and s0[:, 0].min() > 0
