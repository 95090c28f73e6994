"""The survey of the raster without a device: the numpy statement of its definitions (``pairwise_sum_f32``, ``cell_power``,
``cell_floor``, ``cell_mask``, ``bursts`` of pycusdr_amd/channelizer.py), the host back end of ``UniformChannelizer.survey`` under a
cut, the scene that the device test repeats, and the refusals of the Python surface."""
import numpy as np
import pytest

import survey_scene as scene
from pycusdr_amd.channelizer import (BURST, UniformChannelizer, bursts, cell_floor, cell_mask, cell_power, design_taps, pairwise_sum_f32,
                                     unpack_mask)

FS = scene.FS


def tree(p):
    """The definition, recursively, one float32 addition per node."""
    if len(p) == 1:
        return np.float32(p[0])
    h = len(p) // 2
    return np.float32(tree(p[:h]) + tree(p[h:]))


def test_pairwise_sum_is_the_balanced_tree():
    rs = np.random.RandomState(1)
    for n in (1, 2, 4, 8, 64, 1024):
        p = (rs.standard_normal((3, n)) ** 2 * 10.0 ** rs.uniform(-3, 3, (3, n))).astype(np.float32)
        got = pairwise_sum_f32(p)
        assert got.dtype == np.float32 and got.shape == (3,)
        for r in range(3):
            assert got[r] == tree(p[r])
    # float32 at every node, in the tree's order: (2^24 + 1) + (1 + 0) loses both ones, (1 + 1) + (2^24 + 0) keeps them
    assert pairwise_sum_f32(np.array([2.0 ** 24, 1.0, 1.0, 0.0], np.float32)) == np.float32(2.0 ** 24)
    assert pairwise_sum_f32(np.array([1.0, 1.0, 2.0 ** 24, 0.0], np.float32)) == np.float32(2.0 ** 24 + 2.0)
    with pytest.raises(ValueError):
        pairwise_sum_f32(np.ones(12, np.float32))


def test_an_aligned_half_of_a_block_is_its_subtree():
    rs = np.random.RandomState(2)
    p = (rs.standard_normal(256) ** 2).astype(np.float32)
    for n in (256, 64, 8, 2):
        for at in range(0, 256, n):
            lo, hi = pairwise_sum_f32(p[at:at + n // 2]), pairwise_sum_f32(p[at + n // 2:at + n])
            assert pairwise_sum_f32(p[at:at + n]) == np.float32(lo + hi)
    # so partial sums over aligned chunks, summed pairwise again, give the block: the device's split across workgroups
    for chunk in (4, 16, 128):
        assert pairwise_sum_f32(pairwise_sum_f32(p.reshape(-1, chunk))) == pairwise_sum_f32(p)


def test_cell_power_rounds_every_operation_to_float32():
    rs = np.random.RandomState(3)
    y = (rs.standard_normal((4, 64)) + 1j * rs.standard_normal((4, 64))).astype(np.complex64)
    P = cell_power(y, 16)
    assert P.shape == (4, 4) and P.dtype == np.float32
    for k in range(4):
        for s in range(4):
            seg = y[k, 16 * s:16 * s + 16]
            p = [np.float32(np.float32(v.real * v.real) + np.float32(v.imag * v.imag)) for v in seg]
            assert P[s, k] == tree(p)
    with pytest.raises(ValueError):
        cell_power(y, 48)


def test_rank_selection_is_the_sorted_order():
    rs = np.random.RandomState(4)
    P = (rs.standard_normal((6, 16)) ** 2).astype(np.float32)
    P[1, 3:9] = P[1, 0]                     # ties
    P[2] = 0.0                              # an all-zero cell
    P[3, ::2] = 0.0
    for rank in (0, 4, 7, 15):
        f = cell_floor(P, rank)
        assert f.dtype == np.float32 and np.array_equal(f, np.sort(P, axis=1)[:, rank])
        # the counting form of the selection, ties broken by the index: exactly one bin has `rank` values before it
        for s in range(6):
            below = [(np.sum(P[s] < P[s, k]) + np.sum(P[s, :k] == P[s, k])) for k in range(16)]
            assert sorted(below) == list(range(16)) and P[s, below.index(rank)] == f[s]
    assert np.all(cell_floor(P, 9)[2] == 0.0)
    assert not cell_mask(P, cell_floor(P, 4), 4.0)[2].any()          # 0 > 4 * 0 is false: an all-zero cell is empty
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            cell_floor(P, bad)


@pytest.mark.parametrize('M', [8, 16, 32, 64, 256])
def test_mask_packing(M):
    rs = np.random.RandomState(M)
    P = (rs.standard_normal((5, M)) ** 2).astype(np.float32)
    floor = cell_floor(P, M // 4)
    for thr in (1.0, 4.0):
        mask = cell_mask(P, floor, thr)
        assert mask.dtype == np.uint32 and mask.shape == (5, -(-M // 32))
        want = P > (np.float32(thr) * floor)[:, None]
        for s in range(5):
            for k in range(M):
                assert bool((int(mask[s, k // 32]) >> (k % 32)) & 1) == bool(want[s, k])
        if M < 32:
            assert not np.any(mask >> np.uint32(M))                      # unused bits are zero
        assert np.array_equal(unpack_mask(mask, M), want)
        assert want.any() and not want.all()
    # fl(threshold * floor) is a float32 product: a power equal to it is not above it
    P2 = np.full((1, M), np.float32(1.0), np.float32)
    P2[0, 0] = np.float32(1.1) * np.float32(1.0)
    P2[0, 1] = np.nextafter(np.float32(1.1), np.float32(2.0))
    assert np.array_equal(np.flatnonzero(unpack_mask(cell_mask(P2, cell_floor(P2, 2), 1.1), M)[0]), [1])


def pack(occ):
    return cell_mask(occ.astype(np.float32), np.full(len(occ), 0.5, np.float32), 1.0)


def test_bursts():
    occ = np.zeros((12, 8), dtype=bool)
    power = np.arange(96, dtype=np.float32).reshape(12, 8)
    occ[[1, 2, 4, 8], 5] = True             # runs 1..2, 4, 8 of bin 5
    occ[1:4, 2] = True                      # run 1..3 of bin 2
    occ[0, 7] = True
    occ[11, 0] = True                       # a run that ends with the table
    b = bursts(pack(occ), power)
    assert b.dtype == BURST
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in b] == [(7, 0, 0), (2, 1, 3), (5, 1, 2), (5, 4, 4), (5, 8, 8), (0, 11, 11)]
    r = b[1]
    assert r['peak_power'] == power[3, 2] and r['mean_power'] == np.float32(power[1:4, 2].astype(np.float64).mean())
    # hang merges runs that at most `hang` clear cells separate: 1..2 and 4 at hang 1; 8 joins at hang 3
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in bursts(pack(occ), power, hang=1) if r['bin'] == 5] == [(5, 1, 4), (5, 8, 8)]
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in bursts(pack(occ), power, hang=3) if r['bin'] == 5] == [(5, 1, 8)]
    merged = [r for r in bursts(pack(occ), power, hang=1) if r['bin'] == 5][0]
    assert merged['peak_power'] == power[4, 5] and merged['mean_power'] == np.float32(power[1:5, 5].astype(np.float64).mean())
    # min_cells drops short runs, after merging
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in bursts(pack(occ), power, min_cells=2)] == [(2, 1, 3), (5, 1, 2)]
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in bursts(pack(occ), power, hang=1, min_cells=4)] == [(5, 1, 4)]
    # cells count from first_cell
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in bursts(pack(occ), power, first_cell=100)][:2] == [(7, 100, 100), (2, 101, 103)]
    assert len(bursts(pack(np.zeros((3, 8), bool)), power[:3])) == 0
    for kw in (dict(hang=-1), dict(min_cells=0)):
        with pytest.raises(ValueError):
            bursts(pack(occ), power, **kw)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint32), np.ascontiguousarray(v).view(np.uint32))
               for u, v in ((a.power, b.power), (a.floor, b.floor), (a.mask, b.mask)))


def test_host_back_end_under_a_cut():
    rs = np.random.RandomState(5)
    M, D, T, L = 16, 5, 17, 8
    h = rs.uniform(-1, 1, T).astype(np.float32)
    uz = UniformChannelizer(FS, M, D, h, bins=[3, 9], backend='host', max_in=1 << 12)
    uz.set_survey(L, rank=5, threshold=1.5)
    in_base, n = uz.needed_input_cells(0, 8)
    assert (in_base, n) == uz.needed_input(0, 8 * L)
    x = (0.3 * (rs.standard_normal(n + 40) + 1j * rs.standard_normal(n + 40))).astype(np.complex64)
    whole = uz.survey(0, x[:n], 0, 8)
    assert whole.power.shape == (8, M) and whole.floor.shape == (8,) and whole.mask.shape == (8, 1)
    assert (whole.first_cell, whole.cell_frames) == (0, L)
    assert same(whole, uz.survey(0, x, 0, 8))                                # a wider window
    for s in range(8):
        b, c = uz.needed_input_cells(s, 1)
        one = uz.survey(b, x[b:b + c], s, 1)
        assert one.first_cell == s
        assert np.array_equal(one.power, whole.power[s:s + 1]) and np.array_equal(one.floor, whole.floor[s:s + 1])
        assert np.array_equal(one.mask, whole.mask[s:s + 1])
    # the tables are the definitions applied to the outputs of all M bins, whatever is selected
    every = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 12)
    y = every.process(0, x[:n], 0, 8 * L)
    assert np.array_equal(whole.power, cell_power(y, L)) and np.array_equal(whole.floor, cell_floor(whole.power, 5))
    assert np.array_equal(whole.mask, cell_mask(whole.power, whole.floor, 1.5))
    assert np.array_equal(whole.occupied(), whole.power > (np.float32(1.5) * whole.floor)[:, None])
    res, out = uz.survey(0, x[:n], 0, 8, write=True)
    assert same(res, whole) and np.array_equal(out, y[[3, 9]])
    assert np.array_equal(out, uz.process(0, x[:n], 0, 8 * L))


def test_the_scene():
    assert (scene.M, scene.D, len(scene.TAPS), scene.L) == (16, 8, 129, 32)
    uz = UniformChannelizer(FS, scene.M, scene.D, scene.TAPS, backend='host', max_in=1 << 12)
    uz.set_survey(scene.L, threshold=scene.THRESHOLD)                        # rank M / 4
    in_base, n = uz.needed_input_cells(0, scene.NCELLS)
    assert in_base == 0
    res = uz.survey(0, scene.capture(n), 0, scene.NCELLS)
    occupied, judged = scene.expectation()
    # the bins next to a tone, named from the taps: one to either side is 30 dB down, in the transition band; the next are below 90
    assert scene.adjacent(3) == [2, 4] and scene.adjacent(11) == [10, 12]
    assert scene.response(2) < 1e-9 < scene.STOP_BAND < 1e-3 < scene.response(1)
    assert occupied.sum() == 5 and (~judged).sum() == 2 * 3 + 4 * 2 + 2 * 3 + 1 * 2
    # the margins that keep the device's rounding from flipping a bit: set cells above twice the threshold level (and at least 8 times
    # the floor), clear cells below half of it
    level = np.float32(scene.THRESHOLD) * res.floor
    assert np.all(res.power[occupied] > 2 * np.broadcast_to(level[:, None], occupied.shape)[occupied])
    assert np.all(res.power[occupied] >= 8 * np.broadcast_to(res.floor[:, None], occupied.shape)[occupied])
    clear = judged & ~occupied
    assert np.all(res.power[clear] < 0.5 * np.broadcast_to(level[:, None], clear.shape)[clear])
    occ = res.occupied()
    assert np.array_equal(occ[judged], occupied[judged])
    # as bursts: the long tone survives min_cells = 3, the one-cell tone (with its transition cells at most 3 long) needs fewer
    got = res.bursts(min_cells=4)
    assert [r['bin'] for r in got] == [3] and got[0]['first_cell'] <= 2 and got[0]['last_cell'] >= 5
    assert got[0]['peak_power'] == res.power[:, 3].max()
    assert sorted(set(r['bin'] for r in res.bursts())) == sorted(set(np.flatnonzero(occ.any(axis=0))))


def test_every_refusal_is_a_value_error():
    h = design_taps(4)
    uz = UniformChannelizer(FS, 16, 4, h, backend='host', max_in=1 << 12, max_out=1 << 10)
    x = np.zeros(1 << 12, np.complex64)
    with pytest.raises(ValueError):
        uz.survey(0, x, 0, 1)                                                # no survey set
    with pytest.raises(ValueError):
        uz.needed_input_cells(0, 1)
    for L in (3, 12, 2, 1, 1 << 17, -4):
        with pytest.raises(ValueError):
            uz.set_survey(L)
    with pytest.raises(ValueError):
        uz.set_survey(2048)                                                  # longer than max_out
    for rank in (-1, 16):
        with pytest.raises(ValueError):
            uz.set_survey(8, rank=rank)
    for thr in (0.99, 0.0, -4.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            uz.set_survey(8, threshold=thr)
    with pytest.raises(ValueError):
        uz.survey(0, x, 0, 1)                                                # every refusal left it unset
    uz.set_survey(8)
    assert uz.survey(0, x, 0, 2).power.shape == (2, 16)
    for first, n in ((-1, 1), (0, 0), (0, 129), (1 << 60, 1)):               # beyond max_out, beyond out_base * D < 2^62
        with pytest.raises(ValueError):
            uz.survey(0, x, first, n)
    with pytest.raises(ValueError):
        uz.survey(0, x[:10], 0, 2)                                           # the input does not cover the cells
    with pytest.raises(ValueError):
        uz.survey(0, (1234, 10), 0, 1)                                       # device memory on the host back end
    big = UniformChannelizer(FS, 256, 2, h, bins=[0], backend='host', max_in=1 << 24, max_out=1 << 22)
    big.set_survey(4)
    with pytest.raises(ValueError):
        big.survey(0, x, 0, (1 << 18) + 1)                                   # 256 * frames > 2^26
    with pytest.raises(ValueError):
        big.survey(0, x, 0, (1 << 14) + 1)                                   # 256 * cells > 2^22
    uz.set_survey(0)
    with pytest.raises(ValueError):
        uz.survey(0, x, 0, 1)
