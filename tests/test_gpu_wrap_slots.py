"""The slots of a wave of the matrix-core search (wrap_kernels.hpp, k_segw): the planner (fsm_plan, csrc/search_plan.hpp) gives this form a rectangle of its
own -- the group's whole share of bins, up to 32 a chunk, and several slots a wave --, so that a wave now walks from slot to slot with
its fragments, windows and bin tables rebuilt each time.  What a wave keeps from slot to slot must not reach the bits: every
rectangle (MFB_SEG_FSM_RECT = bins,slots, and the planner's default without it) is held to the one-bin, one-slot rectangle, which
carries nothing and which tests/test_gpu_wrap_binloop.py holds to the oracle.  bench_GMSK at 2^18 samples, the smallest block on this
form: 315 complete slots, the last of which reads its fourth segment past the block's end (the wrapped address form of the sample
load).  The rectangle is read once per process: every one runs in a child of its own (tests/children/slots_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'slots_child.py')
KINDS = ('stream', 'zero_segment')
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')
# D = 2: one unrolled pair of bins, kept for two and three slots; 1,315: one wave walks every slot of the block into the wrapped last one
# D = 33: the slots are split over eight groups of 39 or 40, so that chunks of 2, 7 and 40 slots end short; an odd count of bins
# D = 256: bins grouped by XCD, 32 a group; 64,5 asks for more bins than a group of bins holds, so the planner groups the SLOTS instead
# (256 < 8 * 64) and a wave really takes 64 bins: four chunks of bins over slot groups of 39 or 40
# what mfb_get_search_info reports for the planner's default on 256 CUs: the group's 32 bins at D = 256; at D = 33 two chunks of 17,
# halved once by the small-launch rule (one wave per SIMD) after the slots per wave have gone from 5 to 1; at D = 2 one bin
DEFAULT_BINS = {2: 1, 33: 9, 256: 32}
RECTS = {2: ('2,2', '2,3', '1,315', None), 33: ('16,2', '16,40', '33,7', None), 256: ('32,1', '32,5', '64,5', None)}


def _run(jobs):
    """{key: npz of the child}; jobs = {key: (rectangle or None for the default, child arguments, out)}, side by side (at most 16)"""
    assert len(jobs) <= 16
    base = {k: v for k, v in os.environ.items() if k not in DROP}
    procs = {}
    for key, (rect, args, out) in jobs.items():
        env = dict(base, MFB_SEG_WRAP_MFMA='1') if rect is None else dict(base, MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=rect)
        procs[key] = (subprocess.Popen([sys.executable, CHILD] + args + [out], env=env), out)
    res = {}
    try:
        for key, (p, out) in procs.items():
            assert p.wait(timeout=300) == 0, key
            res[key] = dict(np.load(out))
    finally:
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('D', sorted(RECTS))
def test_every_slot_rectangle_scores_the_bits_of_the_one_slot_rectangle(tmp_path, D):
    """Every table is bit-equal to the 1,1 rectangle's and every pick equal, on both inputs; every child has asserted that the search
    ran on the filter side with 256-point segments."""
    rects = ('1,1',) + RECTS[D]
    res = _run({r: (r, ['tables', str(D)], str(tmp_path / f'd{D}_{(r or "default").replace(",", "_")}.npz')) for r in rects})
    ref = res['1,1']
    assert int(ref['bins_per_forward']) == 1
    for rect in RECTS[D]:
        r = res[rect]
        assert int(r['filter_side']) == 1 and int(r['log2L']) == 8, rect
        print(f'D = {D}, rectangle {rect or "default"}: {int(r["bins_per_forward"])} bins per forward transform')
        if rect is None:
            assert int(r['bins_per_forward']) == DEFAULT_BINS[D], (D, int(r['bins_per_forward']))
        for k in KINDS:
            assert r[f'scores_{k}'].shape[0] == D
            assert np.array_equal(r[f'scores_{k}'], ref[f'scores_{k}']), (rect, k)
            assert np.array_equal(r[f'pick_{k}'], ref[f'pick_{k}'], equal_nan=True), (rect, k)


@pytest.mark.gpu
def test_a_batch_of_two_blocks_scores_the_bits_of_the_blocks_one_by_one(tmp_path):
    """Two blocks of 2^18 samples at 33 bins through the batched search under the rectangle 16,3 (a wave's slots stay inside one
    block) against the same two blocks one per call: tables bit-equal, picks equal."""
    r = _run({'batch': ('16,3', ['batch', '33'], str(tmp_path / 'batch.npz'))})['batch']
    assert int(r['filter_side']) == 1 and int(r['log2L']) == 8
    for b in range(2):
        assert r[f'batch_scores{b}'].shape[0] == 33
        assert np.array_equal(r[f'batch_scores{b}'], r[f'single_scores{b}']), b
        assert np.array_equal(r[f'batch_pick{b}'], r[f'single_pick{b}'], equal_nan=True), b
