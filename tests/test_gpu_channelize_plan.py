"""The channeliser's launch plan on the device: the handle launches what csrc/channelize_plan.hpp's ChzGeom says, for the smallest
handle of each kind.  ``info()`` and ``survey_info()`` report the tile that tests/golden/channelize_plans.json records for the plan
(tests/test_channelize_plan_host.py holds the header to that table without a device), and one call of two workgroups plus a ragged
tail equals the same span computed in two calls cut inside a workgroup, bit for bit: grid, tile and window agree with the kernel."""
import json
import os

import numpy as np
import pytest

from pycusdr_amd.channelizer import Channelizer, UniformChannelizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 1.0e6
MAX_IN = 1 << 16
INTEGER, RATIONAL, UNIFORM, SURVEY = range(4)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'channelize_plans.json')) as f:
        fx = json.load(f)
    return [dict(zip(fx['fields'], row)) for row in fx['rows']]


def recorded(golden, kind, U, D, T, M):
    rows = [r for r in golden if (r['kind'], r['U'], r['D'], r['T'], r['M']) == (kind, U, D, T, M)]
    assert rows and len({(r['threads'], r['tile']) for r in rows}) == 1
    return rows[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def noise(rs, n):
    return (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)


def taps_of(rs, T):
    return (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)


def one_call_equals_two(cz, rs, tile, out_base):
    """outputs out_base .. out_base + 2 tile + 5 in one call, and in two calls cut three outputs into the second workgroup"""
    count, cut = 2 * tile + 5, tile + 3
    in_base, n = cz.needed_input(out_base, count)
    assert n <= MAX_IN
    x = noise(rs, n)
    whole = cz.process(in_base, x, out_base, count)
    assert whole.shape == (cz.K, count)
    parts = np.concatenate((cz.process(in_base, x, out_base, cut), cz.process(in_base, x, out_base + cut, count - cut)), axis=1)
    assert np.array_equal(bits(whole), bits(parts))
    assert np.abs(whole).min() > 0                         # (every output was written)


@pytest.mark.parametrize('D, T, lanes', [(23, 7, 256), (41, 1024, 64)])
def test_integer_plan(golden, D, T, lanes):
    want = recorded(golden, INTEGER, 1, D, T, 0)
    assert want['threads'] == want['tile'] == lanes
    rs = np.random.RandomState(D + T)
    cz = Channelizer(FS, D, taps_of(rs, T), [0.0, 1.0e5, -2.5e5], max_in=MAX_IN)
    assert cz.info() == (lanes, T)
    one_call_equals_two(cz, rs, lanes, 7)
    cz.close()


def test_rational_plan(golden):
    U, D, T = 3, 4, 67
    want = recorded(golden, RATIONAL, U, D, T, 0)
    assert want['tile'] == U * want['threads']
    rs = np.random.RandomState(U + D + T)
    cz = Channelizer(FS, D, taps_of(rs, T), [0.0, 1.0e5, -2.5e5], max_in=MAX_IN, interp=U)
    assert cz.info() == (want['tile'], T)
    one_call_equals_two(cz, rs, want['tile'], 7)
    cz.close()


@pytest.mark.parametrize('M, D, T', [(8, 2, 8), (256, 128, 2049)])
def test_uniform_plan(golden, M, D, T):
    want = recorded(golden, UNIFORM, 1, D, T, M)
    rs = np.random.RandomState(M + D + T)
    uz = UniformChannelizer(FS, M, D, taps_of(rs, T), max_in=MAX_IN)
    assert uz.info() == (want['tile'], T)
    assert uz.survey_info()[:2] == (recorded(golden, SURVEY, 1, D, T, M)['tile'], 0)          # (no survey set)
    one_call_equals_two(uz, rs, want['tile'], 7)
    uz.close()


@pytest.mark.parametrize('M, D, T, cell_of', [(8, 2, 8, lambda Fs: Fs // 2), (256, 128, 2049, lambda Fs: 2 * Fs)], ids=['L<Fs', 'L>Fs'])
def test_survey_plan(golden, M, D, T, cell_of):
    """L < Fs: five cells are two workgroups and a tail of one cell, half a workgroup.  L > Fs: a cell is two workgroups, so there
    is no ragged tail to have; three cells against one and two."""
    Fs = recorded(golden, SURVEY, 1, D, T, M)['tile']
    L = cell_of(Fs)
    rows = [r for r in golden if (r['kind'], r['D'], r['T'], r['M'], r['cell_frames']) == (SURVEY, D, T, M, L)]
    assert rows and all(r['C'] == min(L, Fs) for r in rows)
    rs = np.random.RandomState(M + D + T + 1)
    uz = UniformChannelizer(FS, M, D, taps_of(rs, T), bins=[1, 3], max_in=MAX_IN)
    uz.set_survey(L)
    assert uz.survey_info()[:2] == (Fs, L) and uz.info() == (recorded(golden, UNIFORM, 1, D, T, M)['tile'], T)
    first, ncells, cut = 3, (5 if L < Fs else 3), (2 if L < Fs else 1)
    assert L >= Fs or ncells * L == 2 * Fs + L
    in_base, n = uz.needed_input_cells(first, ncells)
    assert n <= MAX_IN
    x = noise(rs, n)
    whole, y = uz.survey(in_base, x, first, ncells, write=True)
    a, ya = uz.survey(in_base, x, first, cut, write=True)
    b, yb = uz.survey(in_base, x, first + cut, ncells - cut, write=True)
    assert whole.power.shape == (ncells, M) and whole.power.min() > 0
    for name in ('power', 'floor', 'mask'):
        assert np.array_equal(bits(getattr(whole, name)), bits(np.concatenate((getattr(a, name), getattr(b, name))))), name
    assert np.array_equal(bits(y), bits(np.concatenate((ya, yb), axis=1)))
    assert np.array_equal(bits(y), bits(uz.process(in_base, x, first * L, ncells * L)))
    uz.close()
