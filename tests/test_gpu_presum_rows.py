"""Partial sums that are not written (seg_kernels.hpp, wrap_kernels.hpp, k_finalize in small_kernels.hpp): the searches that sum a
bin's rows in registers store row 0 of the complete slots only, and k_finalize counts rows >= 1 below the masked tail's first partial
as zeros without reading them.  What those rows hold is then whatever wrote the buffer last, so one handle of 33 bins at 2^18 samples
runs a search after each of: default basis, span basis (6 rows a bin instead of 8), filters again, the two-pass path (every row and
every partial written, another layout), auto again.  The three tables of the default form must be equal bit for bit to each other and
to a fresh handle's; the span and two-pass tables to fresh handles of their own.  With sum_all_masks off the rows are not summed in
registers (per-filter columns): the same steps, the same demand.  A batch of three blocks on a handle that searched on the span basis
before equals the blocks one per call.  One child per case (tests/children/presum_child.py), under a timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'presum_child.py')
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')


def _child(tmp_path, *args):
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    out = str(tmp_path / ('_'.join(args) + '.npz'))
    subprocess.run([sys.executable, CHILD, *args, out], check=True, env=env, timeout=300)
    return dict(np.load(out))


def test_the_default_form_does_not_see_what_other_forms_left_in_the_rows(tmp_path):
    r = _child(tmp_path, 'steps', '1')
    assert int(r['filter_side']) == 1 and int(r['span_rows']) == 6
    assert [str(r[f'path_{k}']) for k in ('default', 'twopass', 'auto')] == ['segment', 'twopass', 'segment']
    fresh = r['fresh_default']
    assert fresh.shape == (33, 8) and fresh[:, 0].min() > 0 and not fresh[:, 1:].any()
    for k in ('default', 'filters', 'auto'):
        assert np.array_equal(r[f'live_{k}'], fresh), k
    assert np.array_equal(r['live_span'], r['fresh_span']) and not np.array_equal(r['live_span'], fresh)
    assert np.array_equal(r['live_twopass'], r['fresh_twopass']) and not np.array_equal(r['live_twopass'], fresh)


def test_per_filter_sums_keep_every_row(tmp_path):
    r = _child(tmp_path, 'steps', '0')
    assert int(r['span_refused']) == 1
    assert [str(r[f'path_{k}']) for k in ('default', 'twopass', 'auto')] == ['segment', 'twopass', 'segment']
    fresh = r['fresh_default']
    assert fresh.shape == (33, 8) and fresh.min() > 0             # a column per filter: no row is summed into another
    for k in ('default', 'filters', 'auto'):
        assert np.array_equal(r[f'live_{k}'], fresh), k
    assert np.array_equal(r['live_twopass'], r['fresh_twopass'])


def test_a_batch_of_three_blocks_equals_the_blocks_one_per_call(tmp_path):
    r = _child(tmp_path, 'batch')
    assert int(r['filter_side']) == 1
    for b in range(3):
        s = r[f'single_scores{b}']
        assert s[:, 0].min() > 0 and not s[:, 1:].any()
        assert np.array_equal(r[f'batch_scores{b}'], s), b
    assert not np.array_equal(r['single_scores0'], r['single_scores1'])
