"""Rational resampling on the raster without a device: ``UniformChannelizer(interp=U, backend='host')`` is the float64 rational
definition (``Channelizer._model_rational``) on the exact raster words, the polyphase collapse that the device kernel computes
(csrc/channelize_uniform_rational_kernels.hpp) is that definition, the plan checks mirror the C ABI's, and the launch plan
(csrc/channelize_plan.hpp) keeps its promises: printed by a stand-alone program (tests/csrc/channelize_uniform_rational_plan_print.cpp,
plain C++, no HIP) and held to properties stated here, not to a recording."""
import itertools
import os
import shutil
import subprocess
from math import gcd

import numpy as np
import pytest

import chur_shapes as cs
from pycusdr_amd import _lib
from pycusdr_amd.channelizer import Channelizer, ChannelizerSource, UniformChannelizer, check_plan_uniform, design_taps, uniform_rate

FS = 1.024e6             # b fs / M quantises to the exact word for every bin of M = 8 and 16 (test_channelizer_uniform_host.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'channelize_uniform_rational_plan_print.cpp')
SHAPES, taps_of = cs.SHAPES, cs.taps_of


def noise(rs, n):
    return (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)


def collapse(h, M, U, D, x_at, out_base, out_count):
    """Branch sums, circular shift, M-point transform, in float64: the issue's three lines.  ``x_at(n)``: the sample at absolute
    position n (an int64 array), zero below 0."""
    T = len(h)
    h64 = h.astype(np.float64)
    y = np.empty((M, out_count), dtype=np.complex128)
    for i in range(out_count):
        m = out_base + i
        q, r = divmod(m * D, U)
        u = np.zeros(M, dtype=np.complex128)
        for p in range(M):
            j = np.arange(p, -(-(T - r) // U), M)                # r + j U < T
            if len(j):
                u[p] = np.sum(h64[r + j * U] * x_at(q - j))
        v = u[(np.arange(M) + q) % M]
        y[:, i] = np.fft.ifft(v) * M
    return y


@pytest.mark.parametrize('M, U, D, T', SHAPES)
@pytest.mark.parametrize('far', [False, True])
def test_the_collapse_is_the_rational_definition(M, U, D, T, far):
    rs = np.random.RandomState(T)
    h = taps_of(rs, U, D, T)
    assert len(h) == T
    nout = 7
    out_base = ((1 << 40) // D + 3) if far else 0
    uz = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 16, interp=U)
    assert uz.interp == U and uz.rational and uz.Tb == -(-T // U) and uz.K == M
    assert [int(w) for w in uz.words] == [(b << 64) // M for b in range(M)]
    in_base, n = uz.needed_input(out_base, nout)
    x = noise(rs, n)
    ref, S = uz.model(in_base, x, out_base, nout)                # Channelizer._model_rational on the words (b << 64) // M
    x128 = x.astype(np.complex128)

    def x_at(pos):
        ok = pos >= 0
        assert np.all(pos[ok] >= in_base) and np.all(pos < in_base + n)
        return np.where(ok, x128[np.where(ok, pos - in_base, 0)], 0.0)

    y = collapse(h, M, U, D, x_at, out_base, nout)
    err = np.abs(y - ref).max(axis=0) / S
    print(f'M {M} U {U} D {D} T {T} out_base {out_base}: worst |collapse - model| / S = {err.max():.2e}')
    assert S.min() > 0 and err.max() <= 1e-12
    assert np.array_equal(uz.process(in_base, x, out_base, nout), ref.astype(np.complex64))


@pytest.mark.parametrize('M, U, D, T', SHAPES[:3])
def test_the_host_back_end_is_the_channelizers_on_the_same_words(M, U, D, T):
    rs = np.random.RandomState(M + T)
    h = taps_of(rs, U, D, T)
    uz = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 14, interp=U)
    cz = Channelizer(FS, D, h, uz.freqs_hz, backend='host', max_in=1 << 14, interp=U)
    assert np.array_equal(uz.words, cz.words)
    for out_base in (0, 11, (1 << 40) // D + 3):
        in_base, n = uz.needed_input(out_base, 60)
        assert (in_base, n) == cz.needed_input(out_base, 60)
        x = noise(rs, n)
        ya, Sa = uz.model(in_base, x, out_base, 60)
        yb, Sb = cz.model(in_base, x, out_base, 60)
        assert np.abs(ya - yb).max() <= 1e-15 * Sa.max() and np.array_equal(Sa, Sb)
        assert np.array_equal(uz.process(in_base, x, out_base, 60), cz.process(in_base, x, out_base, 60))


def test_force_rational_at_interp_1_keeps_the_integer_model():
    rs = np.random.RandomState(3)
    h = rs.uniform(-1, 1, 37).astype(np.float32)
    a = UniformChannelizer(FS, 8, 3, h, backend='host', max_in=1 << 12, force_rational=True)
    b = UniformChannelizer(FS, 8, 3, h, backend='host', max_in=1 << 12)
    assert a.rational and a.interp == 1 and not b.rational and b.interp == 1
    x = noise(rs, 1000)
    assert np.array_equal(a.process(0, x, 0, 200), b.process(0, x, 0, 200))


def test_every_refusal_is_a_value_error():
    ok = dict(nbins=16, decim=5, taps=np.ones(8, np.float32), bins=None, sample_format='cf32', sample_scale=1.0, interp=3)
    M, D, taps, bins, scale = check_plan_uniform(**ok)
    assert (M, D, scale) == (16, 5, 1.0) and list(bins) == list(range(16)) and len(taps) == 8
    bad = [dict(interp=0), dict(interp=-1), dict(interp=33, decim=1000, taps=np.ones(64)),      # U outside 1 .. 32
           dict(decim=49), dict(interp=2, decim=33),                                            # D > U M
           dict(taps=np.ones(3 * 4096 + 1)), dict(interp=32, decim=33, taps=np.ones(32 * 4096 + 1)),     # ceil(T / U) > 4096
           dict(nbins=4), dict(nbins=24), dict(nbins=512),                                      # M outside the set
           dict(decim=6), dict(interp=4, decim=6), dict(interp=6, decim=9),                     # a common factor
           dict(decim=3), dict(decim=2), dict(interp=5, decim=4),                               # U >= D
           dict(taps=np.ones(2)), dict(interp=32, decim=33, taps=np.ones(31)),                  # T < U
           # what the integer plan refuses
           dict(decim=1), dict(decim=0), dict(taps=np.ones(0)), dict(taps=[1.0, np.nan, 1.0]), dict(taps=[np.inf, 1.0, 1.0]), dict(bins=[]),
           dict(bins=list(range(16)) + [0]), dict(bins=[16]), dict(bins=[-9]), dict(bins=[3, 3]), dict(bins=[-1, 15]), dict(bins=[1.5]),
           dict(sample_format='sc32'), dict(sample_format='sc16', sample_scale=0.3), dict(sample_format='sc8', sample_scale=-0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            check_plan_uniform(**{**ok, **kw})
    # the limits themselves pass
    check_plan_uniform(**{**ok, 'decim': 47})                                                   # D = U M - 1 (48 has the factor 3)
    check_plan_uniform(**{**ok, 'interp': 32, 'decim': 511, 'taps': np.ones(32 * 4096)})
    check_plan_uniform(**{**ok, 'interp': 3, 'decim': 4, 'taps': np.ones(3)})
    for kw in bad[:8]:
        with pytest.raises(ValueError):
            UniformChannelizer(FS, **{k: v for k, v in {**ok, **kw}.items() if k not in ('sample_format', 'sample_scale')}, backend='host')
    uz = UniformChannelizer(FS, 16, 5, np.ones(8, np.float32), backend='host', interp=3)
    with pytest.raises(ValueError, match='rational'):
        uz.set_survey(8)
    with pytest.raises(ValueError):
        uz.survey(0, np.zeros(64, np.complex64), 0, 1)
    forced = UniformChannelizer(FS, 16, 5, np.ones(8, np.float32), backend='host', force_rational=True)
    with pytest.raises(ValueError, match='rational'):
        forced.set_survey(8)
    UniformChannelizer(FS, 16, 5, np.ones(8, np.float32), backend='host').set_survey(8)         # the integer plan keeps its survey


def test_uniform_rate():
    assert uniform_rate(2.4e6, 153600, 64) == (8, 125)
    assert uniform_rate(1.024e6, 64000, 16) == (1, 16)
    assert uniform_rate(3.0e6, 153600, 64) == (32, 625)
    assert uniform_rate(307200, 153600, 8) == (1, 2)
    assert uniform_rate(949200 * 25 // 16, 949200, 8) == (16, 25)
    for fs_in, fs_out, M in ((153600, 2.4e6, 64), (1.0e6, 1.0e6, 8),          # no reduction
                             (2.0e6, 153600, 64),                             # 48 / 625: U > 32
                             (2.4e6, 153600, 8),                              # 8 / 125: D > U M = 64
                             (1.024e6, 1000, 256),                            # 1 / 1024: D > M
                             (2.4e6, 153600, 48)):                            # no such raster
        with pytest.raises(ValueError):
            uniform_rate(fs_in, fs_out, M)
    U, D = uniform_rate(2.4e6, 153600, 64)
    check_plan_uniform(64, D, design_taps(D, interp=U), None, 'cf32', 1.0, interp=U)


@pytest.mark.parametrize('M, U, D, T', SHAPES)
def test_needed_input_is_the_brute_force_enumeration(M, U, D, T):
    uz = UniformChannelizer(FS, M, D, np.ones(T, np.float32), backend='host', interp=U, max_in=1 << 20)
    Tb = -(-T // U)
    for out_base, n in ((0, 1), (0, 40), (1, 1), (3, 5), (U, U), (U + 1, 2 * U + 1), (1000, 77), ((1 << 40) // D + 3, 9)):
        q = [(m * D) // U for m in range(out_base, out_base + n)]
        first = max(0, min(q) - (Tb - 1))
        assert uz.needed_input(out_base, n) == (first, max(q) - first + 1), (out_base, n)
        # every tap of every output is inside, none reads past q
        reads = [qm - j for m, qm in zip(range(out_base, out_base + n), q) for j in (0, -(-(T - (m * D) % U) // U) - 1)]
        assert first <= max(0, min(reads)) and max(reads) == max(q)
    with pytest.raises(ValueError):
        uz.needed_input(-1, 1)


def test_a_source_takes_it():
    uz = UniformChannelizer(FS, 8, 25, design_taps(25, interp=16), bins=[1, 5], backend='host', max_in=1 << 14, max_out=1 << 12, interp=16)
    src = ChannelizerSource(uz, 1, None, 1024, 128, 2, 3)
    assert len(src) == 3 and src.window_input(1) == uz.needed_input(src.window_base(1), src.count)
    with pytest.raises(ValueError, match="not 'hip'"):
        next(iter(src))


def test_the_binding_and_the_library_have_the_entry_point():
    assert 'mfb_uniform_channelizer_set_plan_rational' in _lib.PROTOTYPES
    lib = _lib.load()
    assert hasattr(lib, 'mfb_uniform_channelizer_set_plan_rational') and lib.mfb_abi_version() == 9
    p = (np.ones(4, np.float32)).ctypes.data
    assert lib.mfb_uniform_channelizer_set_plan_rational(None, 1, 2, p, 3, p, 1, 0, 1.0) == _lib.MFB_ERR_ARG


# ---- the plan header
GRID = [(M, U, D, T) for M in (8, 16, 32, 64, 128, 256) for U in (1, 2, 3, 8, 31, 32)
        for D in sorted({U + 1, 2 * U + 1, U * M // 2 + 1, U * M - 1, U * M}) if D > U and gcd(U, D) == 1 and D >= 2
        for T in sorted({U, U + 1, 5 * U + 3, U * M, U * M + 1, 1000 * U + 7, 4096 * U - 5, 4096 * U})]


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path_factory.mktemp('chur_plan') / 'channelize_uniform_rational_plan_print'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', SRC, '-o', str(exe)], capture_output=True,
                           text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    calls = [(0, 1), (0, 300), (7, 129), ((1 << 40) // 3 + 1, 515)]
    tuples = [(M, U, D, T, ob, oc) for (M, U, D, T), (ob, oc) in itertools.product(GRID, calls)]
    got = []
    for at in range(0, len(tuples), 500):
        run = subprocess.run([str(exe)] + [':'.join(str(v) for v in t) for t in tuples[at:at + 500]], capture_output=True, text=True,
                             timeout=60)
        assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
        got += [{k: int(v) for k, v in (kv.split('=') for kv in line.split())} for line in run.stdout.strip().splitlines()]
    assert len(got) == len(tuples)
    return got


def test_the_plan_header_keeps_its_promises(printed):
    assert len(GRID) > 500 and {g[0] for g in GRID} == {8, 16, 32, 64, 128, 256}
    tiles = set()
    for g in printed:
        M, U, D, T, F = g['M'], g['U'], g['D'], g['T'], g['F']
        Tb = -(-T // U)
        assert g['kind'] == 5 and (g['gU'], g['gD'], g['gT'], g['gM'], g['Tb'], g['threads']) == (U, D, T, M, Tb, 256), g
        assert g['tile'] == F >= 1 and F * M % 256 == 0, g
        assert g['span'] == g['S'] == cs.brute_span(U, D, T, F), g
        assert g['lds'] == g['lds_bytes'] == (g['span'] + F * (M + 1) + M) * 8 <= g['budget'] == cs.LDS_BUDGET, g
        # the largest F of the rule's ladder that fits: the next larger one does not
        assert F == cs.plan_frames(M, U, D, T), g
        bigger = [f for f in cs.ladder(M) if f > F]
        assert not bigger or cs.lds_bytes(M, U, D, T, bigger[0]) > g['budget'], g
        ob, oc = g['out_base'], g['out_count']
        assert g['grid'] == -(-oc // F)
        assert g['first'] == (ob * D) // U - (Tb - 1) and g['last'] == ((ob + oc - 1) * D) // U, g
        tiles.add(F)
    assert {4, 16, 128} <= tiles, tiles
    # U = 1 is the integer plan's geometry
    for g in printed:
        if g['U'] == 1:
            assert g['span'] == (g['F'] - 1) * g['D'] + g['T']
