"""The stream-stage kernels (csrc/stream_kernels.hpp) at their launch-geometry edges, through the seam ``MFBank.debug_stream_stages``
on injected symbol decisions and centres: the strided sweep's later trips, counts that are no multiple of four, overlap_offset
1 ... 31, the tail branches one by one, the limits of the LDS LUT copies, batches of 1 ... 64 blocks chained on the device's carry
(k_stream_align); tap counts on the word borders, streams that reach back over many blocks, saturated hit and edge lists, hits at
both ends, sync_valid (k_stream_search) -- and the byte forms k_stream_sync / k_stream_ring / k_stream_edges in a child process.
Every case is one of tests/stream_cases.py, whose ``reach`` conditions tests/test_stream_model.py proves on the model alone; here
every block's status must be the model's (0 exactly where the model says irregular) and every block the device kept must equal the
host code's results: integer kernels, so everything with np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_cases as sc
from pycusdr_amd.mfbank import MFBank

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'stream_child.py')


@pytest.fixture(scope='module')
def banks():
    made = {}

    def get(log2N):
        if log2N not in made:
            made[log2N] = MFBank(log2N, 4, 2)
        return made[log2N]
    yield get
    for b in made.values():
        b.close()


def _run(banks, name):
    c = sc.case(name)
    results, recs = sc.drive(c, banks(c.log2N))
    c.reach(results)                     # (the branch is reached: also proven without a GPU)
    assert len(results) == len(recs)
    for i, (res, rec) in enumerate(zip(results, recs)):
        sc.check_batch(res, rec, (name, i))
    return results, recs


ALIGN = [n for n in sc.CASES if n.split('-')[0] in ('second_stride', 'count_tails', 'tiny', 'offset_limits', 'tails_seed', 'tails_batch',
                                                    'tails_noerr', 'lut_limits', 'batch_sizes')]
SEARCH = [n for n in sc.CASES if n not in ALIGN]


@pytest.mark.parametrize('name', ALIGN)
def test_align_equals_the_host_code(banks, name):
    """A12 / A13 (k_stream_align)."""
    _run(banks, name)


@pytest.mark.parametrize('name', SEARCH)
def test_search_equals_np_convolve(banks, name):
    """A14 (k_stream_search): hits, would-be stash edges, and the ring through the next batch's hits."""
    _run(banks, name)


def test_every_case_is_run():
    assert sorted(ALIGN + SEARCH) == sorted(sc.CASES) and set(sc.BYTE_CASES) <= set(SEARCH)


def test_byte_forms_equal_the_model_and_the_packed_kernel(banks, tmp_path):
    """k_stream_sync / k_stream_ring / k_stream_edges (MFB_STREAM_UNPACKED, read once per process: one child) on the word-border
    templates, the long reach back and the block with more header hits than edge candidates."""
    out = str(tmp_path / 'bytes.npz')
    p = subprocess.run([sys.executable, CHILD, out], env=dict(os.environ, MFB_STREAM_UNPACKED='1'), timeout=300)
    assert p.returncode == 0
    got = dict(np.load(out))
    for name in sc.BYTE_CASES:
        c = sc.case(name)
        results = sc.model_results(name)
        packed = sc.drive(c, banks(c.log2N))[1]
        for i, res in enumerate(results):
            rec = {k: got[f'{name}|{i}|{k}'] for k in packed[i]}
            sc.check_batch(res, rec, (name, i, 'bytes'))
            sc.check_batch(res, packed[i], (name, i, 'packed'))
            for k in sc.SCALARS:
                assert np.array_equal(rec[k], packed[i][k]), (name, i, k)
