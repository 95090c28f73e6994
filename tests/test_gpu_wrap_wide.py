"""Rectangles of 64 bins in the matrix-core search (wrap_kernels.hpp, k_segw; the planner is fsm_plan in csrc/search_plan.hpp): a wave that
builds a slot's fragments once for 64 bins instead of 32, over groups of slots, over eight groups of bins or over four.  The bits
must not know: every table is equal to the one-bin, one-slot rectangle's of the same D on both inputs of the child, picks equal.
bench_GMSK at 2^18 samples (315 complete slots), the smallest block on this form; one child per rectangle
(tests/children/slots_child.py, as tests/test_gpu_wrap_slots.py runs it), the 1,1 child of a D beside it.

Forced 64,1 (MFB_SEG_FSM_RECT):
  D = 256   slot groups (256 < 8 * 64), four chunks of 64 bins, one slot a wave
  D = 257   slot groups; five chunks, the last of one bin
  D = 512   bin groups of exactly 64
  D = 520   bin groups of 65: a 64-bin chunk and a one-bin chunk, the odd end of the unrolled pair
The planner's default:
  D = 1024  bin groups of 128: two chunks of 64 where the launch keeps four rounds of waves (5040 one-slot waves against 16 per CU)
  D = 1040  bin groups of 130: three chunks of 44 under the same rule
  D = 256 and 255 at 2^20 samples (1260 slots; tests/children/wide_child.py): FOUR groups of 64 bins (of 63, 64, 64 and 64), each on
            a pair of XCDs -- the plan of the 2^20-sample, 256-bin search, which no smaller block reaches
What the default reports is computed here from the planner's rule and the device's CU count, not written down for one device."""
import os
import subprocess
import sys

import numpy as np
import pytest

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'slots_child.py')
WIDE_CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'wide_child.py')
KINDS = ('stream', 'zero_segment')
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')
NFULL = {18: 315, 20: 1260}       # complete slots of a block of this bank


def _ceil(a, b):
    return (a + b - 1) // b


def planned_bins(D, cus, nfull=NFULL[18]):
    """bins per forward transform of the planner's default for k_segw (nfull >= 64), restated from its rule"""
    # the wide plan: groups of bins -- four up to 256 bins, else eight --, chunks of at most 64, four one-slot waves for every SIMD
    if D >= 128:
        nsg = 4 if D <= 256 else 8
        share = _ceil(D, nsg)
        chunks = _ceil(share, 64)
        if nsg * chunks * nfull >= 4 * 4 * cus:
            return _ceil(share, chunks)
    # the narrow plan: groups of bins from 16 bins a group, chunks of at most 32, five slots a wave; a wave for every SIMD comes first
    by_bins = D >= 8 * 16
    share, glen = (_ceil(D, 8), nfull) if by_bins else (D, _ceil(nfull, 8))
    fb, fs = _ceil(share, _ceil(share, 32)), min(5, glen)
    waves = lambda: 8 * _ceil(share, fb) * _ceil(glen, fs)          # noqa: E731
    while fs > 1 and waves() < 4 * cus:
        fs = (fs + 1) >> 1
    while fb > 1 and waves() < 4 * cus:
        fb = (fb + 1) >> 1
    return fb


def _pair(tmp_path, D, rect, log2N=18):
    """(npz of the 1,1 child, npz of the child under `rect`; None = the planner's default), the two side by side"""
    base = {k: v for k, v in os.environ.items() if k not in DROP}
    procs = []
    for r in ('1,1', rect):
        env = dict(base, MFB_SEG_WRAP_MFMA='1') if r is None else dict(base, MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=r)
        out = str(tmp_path / f'd{D}_{(r or "default").replace(",", "_")}.npz')
        cmd = [CHILD, 'tables', str(D), out] if log2N == 18 else [WIDE_CHILD, str(log2N), str(D), out]
        procs.append((subprocess.Popen([sys.executable] + cmd, env=env), out))
    res = []
    try:
        for p, out in procs:
            assert p.wait(timeout=300) == 0, out
            res.append(dict(np.load(out)))
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
    return res


def _same_bits(D, ref, r, rect):
    assert int(ref['bins_per_forward']) == 1
    assert int(r['filter_side']) == 1 and int(r['log2L']) == 8, rect
    for k in KINDS:
        assert r[f'scores_{k}'].shape[0] == D
        assert np.array_equal(r[f'scores_{k}'], ref[f'scores_{k}']), (rect, k)
        assert np.array_equal(r[f'pick_{k}'], ref[f'pick_{k}'], equal_nan=True), (rect, k)


def test_the_rule_restated_here_gives_the_narrow_plan_where_the_launch_is_short():
    """On 256 CUs at 2^18 samples: 1260 waves of 64 x 1 at D = 256 are under 4096, so the default there stays 32 bins (and 9 at D = 33,
    1 at D = 2, as tests/test_gpu_wrap_slots.py asserts on the device); 5040 at D = 1024 and 7560 at D = 1040 are not."""
    assert [planned_bins(D, 256) for D in (2, 33, 256)] == [1, 9, 32]
    assert [planned_bins(D, 256) for D in (1024, 1040)] == [64, 44]
    assert [planned_bins(D, 256, nfull=1260) for D in (127, 128, 255, 256, 257, 384)] == [32, 32, 64, 64, 33, 48]
    assert planned_bins(1024, 320) == 32              # 5040 waves under 16 x 320: the narrow plan, four chunks of 32


@pytest.mark.gpu
@pytest.mark.parametrize('D', [256, 257, 512, 520])
def test_forced_64_bin_rectangles_score_the_bits_of_the_one_bin_rectangle(tmp_path, D):
    ref, r = _pair(tmp_path, D, '64,1')
    assert int(r['bins_per_forward']) == 64
    _same_bits(D, ref, r, '64,1')


@pytest.mark.gpu
@pytest.mark.parametrize('D', [1024, 1040])
def test_the_planners_default_scores_the_bits_of_the_one_bin_rectangle(tmp_path, D):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref, r = _pair(tmp_path, D, None)
    want = planned_bins(D, cus)
    print(f'D = {D}, {cus} CUs: {int(r["bins_per_forward"])} bins per forward transform (rule: {want})')
    if D == 1024 and 5040 >= 16 * cus:
        assert want == 64
    assert int(r['bins_per_forward']) == want, (D, cus, int(r['bins_per_forward']), want)
    _same_bits(D, ref, r, 'default')


@pytest.mark.gpu
@pytest.mark.parametrize('D', [255, 256])
def test_four_groups_of_bins_score_the_bits_of_the_one_bin_rectangle(tmp_path, D):
    """The planner's default at 2^20 samples: 4 x 1260 = 5040 one-slot waves of 64 bins, the wide plan wherever 16 waves a CU are
    no more than that (256 CUs: 4096)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref, r = _pair(tmp_path, D, None, log2N=20)
    want = planned_bins(D, cus, nfull=NFULL[20])
    print(f'D = {D}, 2^20 samples, {cus} CUs: {int(r["bins_per_forward"])} bins per forward transform (rule: {want})')
    if 5040 >= 16 * cus:
        assert want == 64
    assert int(r['bins_per_forward']) == want, (D, cus, int(r['bins_per_forward']), want)
    _same_bits(D, ref, r, 'default')
