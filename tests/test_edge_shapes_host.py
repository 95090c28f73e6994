"""The premises of the GPU edge tests (test_gpu_modulator_edges.py, test_gpu_channelizer_shapes.py), without a GPU: every shape of
tests/edge_shapes.py reaches the branch, tile or boundary it is listed for, and neither fp32 quotient estimate is ever off by more
than the one step its kernel corrects.  A later change of a shape that made a GPU test vacuous fails here."""
import numpy as np
import pytest

import edge_shapes as es
import modulator_model as mm


def test_the_shapes_the_suite_had_never_correct():
    """Why the new shapes are needed: 2, 5, 16 and 128 samples per symbol estimate every k a handle allows exactly."""
    for sps in (2, 5, 16, 128):
        n = min(es.MOD_MAX_SAMPLES, es.MOD_MAX_FRAME_BITS * sps)
        _, r = es.estimate(np.arange(n), sps)
        assert r.min() >= 0 and r.max() < sps, sps


@pytest.mark.parametrize('sps', es.MOD_UP_SPS)
def test_modulator_upward_cases_reach_the_branch(sps):
    for bits in es.MOD_UP_BITS:
        q, r = es.estimate(np.arange(bits * sps), sps)
        up = np.flatnonzero(r >= sps)
        assert up.size >= 1 and r.min() >= 0, (sps, bits)
        assert np.all(r[up] < 2 * sps)                      # one step mends it
        if sps == 41:
            assert up[0] == 41                                # the first of all: k = sps


def test_modulator_downward_case_reaches_the_branch():
    sps, bits = es.MOD_DOWN
    assert bits <= es.MOD_MAX_FRAME_BITS and bits * sps <= es.MOD_MAX_SAMPLES
    q, r = es.estimate(np.arange(bits * sps), sps)
    down = np.flatnonzero(r < 0)
    assert down.size >= 1 and down[0] == 8487929
    assert np.all(r[down] >= -sps)
    assert down[0] >= bits * sps - (1 << 16)                 # inside the tail whose samples the GPU test evaluates


def test_no_modulator_estimate_is_off_by_more_than_one():
    """Every sps, at both ends of every symbol a handle allows: k = s sps (the true remainder 0, where a low estimate shows) and
    k = s sps - 1 (the true remainder sps - 1, where a high one shows).  Between the two the estimate is monotone in k."""
    first_up, first_down = {}, {}
    for sps in range(2, es.MOD_MAX_SPS + 1):
        nsym = min(es.MOD_MAX_FRAME_BITS, es.MOD_MAX_SAMPLES // sps)
        s = np.arange(1, nsym + 1, dtype=np.int64)
        k = s * sps
        k = k[k < es.MOD_MAX_SAMPLES]
        s = s[:len(k)]
        q, _ = es.estimate(k, sps)
        assert np.all(np.abs(q - s) <= 1), sps
        if np.any(q < s):
            first_up[sps] = int(k[np.argmax(q < s)])
        q, _ = es.estimate(k - 1, sps)
        assert np.all(np.abs(q - (s - 1)) <= 1), sps
        if np.any(q > s - 1):
            first_down[sps] = int(k[np.argmax(q > s - 1)] - 1)
    assert min(first_up) == 41 and first_up[41] == 41
    assert sorted(first_up)[:6] == [41, 47, 55, 61, 82, 83]
    assert set(es.MOD_UP_SPS) <= set(first_up)
    best = min(first_down, key=first_down.get)
    assert (best, first_down[best]) == (255, 8487929) and es.MOD_DOWN[0] == 255


@pytest.mark.parametrize('sps', es.MANY_SPS)
@pytest.mark.parametrize('min_bits', [1, 2])
def test_many_frames_put_boundaries_on_the_chosen_threads(sps, min_bits):
    lengths, residues = es.many_frame_lengths(sps, min_bits, 11)
    assert es.MANY_FRAMES <= len(lengths) <= 4096 and min(lengths) >= min_bits and max(lengths) <= 5
    off = np.cumsum([mm.layout(n * sps, 0, 0)[1] for n in lengths])[:-1]
    hit = set((off % es.MOD_WORKGROUP).tolist())
    assert set(residues) <= hit, (sps, min_bits)
    if sps % 2:
        assert {255, 0, 1} <= hit                             # sample 255, 256 and 257 of a workgroup
    # dozens of frames in a workgroup: the third bisection chooses among many
    per_group = np.bincount(off // es.MOD_WORKGROUP)
    assert per_group[:-1].min() >= 12 and per_group.max() >= 24, (per_group.min(), per_group.max())


def test_scan_lengths_cover_the_tile_edges():
    L = set(es.SCAN_LENGTHS)
    assert {es.MOD_TILE - 1, es.MOD_TILE, es.MOD_TILE + 1, 2 * es.MOD_TILE, 3 * es.MOD_TILE + 1, es.MOD_MAX_FRAME_BITS} <= L
    assert {n % 4 for n in L if n > 4} == {0, 1, 2, 3}       # a last thread with 1, 2, 3 and 4 live symbols
    assert es.MOD_MAX_FRAME_BITS == 128 * es.MOD_TILE
    assert sum(es.SCAN_LENGTHS) * es.SCAN_SPS <= 1 << 20
    d = mm.quantise(np.array(es.SCAN_DPHI))
    d = [int(v) for v in d]
    assert d[0] == 0 and 0 < d[1] < 1 << 54 and d[2] > (1 << 64) - (1 << 54) and d[3] == 1 << 63
    # in one of the rotations the longest frame takes the increment whose step wraps at every symbol
    at = es.SCAN_LENGTHS.index(es.MOD_MAX_FRAME_BITS)
    assert any(es.SCAN_DPHI[(at + rot) % len(es.SCAN_DPHI)] < 0 for rot in es.SCAN_ROTATIONS)


def test_pad_cases_hold_both_kinds_of_frame():
    for pad, min_len in es.PADS:
        pre = [mm.layout(n * es.PAD_SPS, pad, min_len)[0] for n in es.PAD_BITS]
        if min_len:
            assert min(pre) == 0 and sum(p > 0 for p in pre) >= 2, (pad, min_len, pre)
        else:
            assert max(pre) == 0
        assert (pad % 256, min_len % 256) != (0, 0)


@pytest.mark.parametrize('D,T,tile,corr', es.CHZ_SHAPES)
def test_channeliser_shapes_have_the_listed_tile_and_correction(D, T, tile, corr):
    assert es.chz_threads(D, T) == tile
    assert D * es.chz_row_len(tile, D, T) * 8 <= es.CHZ_LDS_BUDGET
    if tile < 256:
        assert D * es.chz_row_len(2 * tile, D, T) * 8 > es.CHZ_LDS_BUDGET
    span = es.chz_span(D, T)
    q, r = es.estimate(np.arange(span), D)
    assert r.min() >= 0
    up = np.flatnonzero(r >= D)
    assert (up.size >= 1) == corr, (D, T, up[:4])
    if corr:
        assert up[0] == D and np.all(r[up] < 2 * D)
    # where the corrected position lands is inside the image
    assert np.all(np.arange(span) // D < es.chz_row_len(tile, D, T))


def test_tile_ranges_are_the_ones_the_shapes_sit_at():
    assert [D for D in range(2, 65) if es.chz_threads(D, 16) == 128] == list(range(24, 48))
    assert [D for D in range(2, 65) if es.chz_threads(D, 1024) == 128] == list(range(21, 41))
    assert es.chz_threads(23, 7) == 256 and es.chz_threads(64, 1024) == 64
    T = sorted({t for _, t, _, _ in es.CHZ_SHAPES})
    assert {es.CHZ_UNROLL - 1, es.CHZ_UNROLL, es.CHZ_UNROLL + 1, 2 * es.CHZ_UNROLL, es.CHZ_MAX_TAPS} <= set(T)


def test_no_channeliser_estimate_is_off_by_more_than_one():
    """Every D over the largest span a workgroup stages (T = 1024); only 41, 47, 55 and 61 ever correct, and only upward."""
    corrected = []
    for D in range(2, es.CHZ_MAX_DECIM + 1):
        span = max(es.chz_span(D, T) for T in (1, es.CHZ_MAX_TAPS))
        assert span < 1 << 15
        p = np.arange(span)
        q, r = es.estimate(p, D)
        assert np.all(np.abs(q - p // D) <= 1), D
        assert r.min() >= 0, D
        if r.max() >= D:
            corrected.append(D)
            assert np.argmax(r >= D) == D
    assert corrected == [41, 47, 55, 61]
    assert {D for D, _, _, c in es.CHZ_SHAPES if c} == set(corrected)


def test_channel_count_plans_reach_every_group_size():
    def groups(n):
        return [4] * (n // 4) + ([2] if n & 2 else []) + ([1] if n & 1 else [])
    cplx = [g for c, _ in es.CHZ_COUNTS for g in groups(c)]
    real = [g for _, r in es.CHZ_COUNTS for g in groups(r)]
    assert {1, 2, 4} <= set(cplx) and {1, 2, 4} <= set(real)
    assert any(c and c & 2 and not c & 1 for c, _ in es.CHZ_COUNTS)          # 2, 6: a pair and no single
    assert any(c and c % 4 == 0 for c, _ in es.CHZ_COUNTS) and any(r and r % 4 == 0 for _, r in es.CHZ_COUNTS)
    for i, (c, r) in enumerate(es.CHZ_COUNTS):
        assert 1 <= c + r <= 16
        real_at = es.scatter_real(c, r, i)
        assert real_at.sum() == r
        order = list(np.flatnonzero(~real_at)) + list(np.flatnonzero(real_at))
        if c and r:
            assert order != sorted(order) and np.any(np.diff(np.flatnonzero(real_at)) > 1)


def test_cut_and_roomy_shapes():
    tiles = {es.chz_threads(D, T) for D, T, _ in es.CHZ_CUT_SHAPES}
    assert tiles == {128, 64}                                 # the 256-lane tile has test_pure_function_of_position
    assert {f for _, _, f in es.CHZ_CUT_SHAPES} == {'cf32', 'sc16'}
    R = es.CHZ_ROOMY
    D, T, K = R['A']
    assert T < R['max_taps'] and K < R['max_channels']        # tap_stride is not the plan's T
    assert es.chz_threads(D, T) == 128 and es.chz_threads(*R['B'][:2]) == 256
