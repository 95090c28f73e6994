"""The 256-point search with the wrap-around energy on the matrix cores (wrap_kernels.hpp, k_segw) against the same search on the
vector ALUs (segf_body, MFB_SEG_WRAP_MFMA=0) and against the oracle, on adversarial blocks (tests/children/wrap_child.py).
MFB_SEG_WRAP_MFMA is read once per process: each form runs in a child of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mfbank_oracle as orc

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'wrap_child.py')


def _run(tmp_path, name, log2N, D, rect=None):
    res = {}
    for form in ('0', '1'):
        out = str(tmp_path / f'wrap{form}.npz')
        env = dict(os.environ, MFB_SEG_WRAP_MFMA=form)
        for k in ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP'):
            env.pop(k, None)
        if rect:           # a wave's rectangle (bins, slots)
            env['MFB_SEG_FSM_RECT'] = rect
        subprocess.run([sys.executable, CHILD, name, str(log2N), str(D), out], check=True, env=env, timeout=600)
        res[form] = dict(np.load(out))
    return res['0'], res['1']


def _kinds(r):
    return sorted(k[len('scores_'):] for k in r if k.startswith('scores_'))


def _per_bin_err(got, ref):
    """error of every bin at or above 1e-4 of the block's largest score, relative to that bin's own score"""
    g, s = got[:, 0].astype(np.float64), ref[:, 0]
    keep = s >= 1e-4 * s.max()
    return np.abs(g[keep] - s[keep]) / s[keep]


@pytest.mark.gpu
def test_wrap_mfma_against_the_oracle_on_adversarial_blocks(tmp_path):
    """Bursts at every phase of the wrap window on a -60 dB floor, tones on and between bins, a block that is zero but for one
    segment, a peak-clipped stream: per bin the matrix-core form is within 1e-5 of the oracle (fp64 inverse transforms of length N)
    and no more than twice as far from it as the vector form (plus fp32 rounding of the score itself)."""
    from pycusdr_amd.protocol import loadProtocol
    from pycusdr_amd import config as cfg
    name, log2N, D = 'bench_GMSK', 18, 64
    valu, mfma = _run(tmp_path, name, log2N, D)
    assert int(mfma['filter_side']) == 1 and int(mfma['log2L']) == 8
    N = 1 << log2N
    conf = cfg.bench_config(name, blockSize=log2N, doppCarrierSteps=D)
    _, masks = loadProtocol(name)(conf=conf).get_filter(N, 16, 3)
    worst, clear = {}, {}
    for k in _kinds(mfma):
        ref = orc.doppler_scores(mfma[f'X_{k}'], masks, mfma['shifts'], True)
        em, ev = _per_bin_err(mfma[f'scores_{k}'], ref), _per_bin_err(valu[f'scores_{k}'], ref)
        worst[k] = (float(em.max()), float(ev.max()))
        top = np.sort(ref[:, 0])[::-1]
        # the pick interpolates between the two largest bins: a tone on a bin leaves its two neighbours tied for second, and
        # fp32 rounding decides which side the pick falls -- compared only where the top three are apart
        clear[k] = top[0] - top[1] > 1e-4 * top[0] and top[1] - top[2] > 1e-4 * top[1]
    print('per-bin relative error (matrix cores, vector ALUs):', worst)
    for k in _kinds(mfma):
        assert not np.array_equal(mfma[f'scores_{k}'], valu[f'scores_{k}']), k
        if clear[k]:
            assert abs(float(mfma[f'pick_{k}'][0]) - float(valu[f'pick_{k}'][0])) < 1e-3, k
    for k, (em, ev) in worst.items():
        assert em <= 1e-5, (k, em, ev)
        assert em <= 2 * ev + 2e-7, (k, em, ev)


@pytest.mark.gpu
@pytest.mark.parametrize('log2N,D', [(20, 256), (20, 1024)])
def test_wrap_mfma_matches_the_vector_form_at_full_size(tmp_path, log2N, D):
    """C2 and C3 shapes: the two forms agree to fp32 rounding on every input, with the same pick."""
    valu, mfma = _run(tmp_path, 'bench_GMSK', log2N, D)
    assert not np.array_equal(valu['scores_stream'], mfma['scores_stream'])           # two forms ran
    for k in _kinds(mfma):
        a, b = valu[f'scores_{k}'].astype(np.float64), mfma[f'scores_{k}'].astype(np.float64)
        assert np.abs(a - b).max() / a.max() < 2e-6, k
        assert abs(float(mfma[f'pick_{k}'][0]) - float(valu[f'pick_{k}'][0])) < 1e-3, k
        assert np.all(b[:, 1:] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize('name,log2N,D,rect', [('bench_BPSK', 18, 40, '8,1'), ('bench_GMSK', 17, 64, '16,1'), ('bench_GMSK', 16, 64, None)])
def test_vector_form_where_the_matrix_form_does_not_apply(tmp_path, name, log2N, D, rect):
    """The BPSK bank (80 taps, 16 filter rows: two column tiles) and blocks below 2^18 samples stay on segf_body -- whatever the
    rectangle, so that the choice never depends on the grid: both settings give the same bits."""
    valu, mfma = _run(tmp_path, name, log2N, D, rect=rect)
    for k in _kinds(mfma):
        assert np.array_equal(valu[f'scores_{k}'], mfma[f'scores_{k}']), k


@pytest.mark.gpu
def test_wrap_mfma_bits_do_not_depend_on_the_rectangle(tmp_path):
    """The matrix-core form scores a (block, shift) from the bin's own tables in a fixed order: one-bin and sixteen-bin rectangles
    give the same bits."""
    res = []
    for rect in ('1,1', '16,1', '5,3'):
        d = tmp_path / rect.replace(',', '_')
        d.mkdir()
        res.append(_run(d, 'bench_GMSK', 18, 48, rect=rect)[1])
    for r in res[1:]:
        for k in _kinds(r):
            assert np.array_equal(r[f'scores_{k}'], res[0][f'scores_{k}']), k
