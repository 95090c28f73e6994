"""Rational resampling in the channeliser, the host side: the float64 model against a brute-force zero-stuff / convolve / stride
statement of the definition, the integer plan untouched, ``design_taps``, ``needed_input``, ``check_plan``, ``factor_rate`` and the
new entry point's presence.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd.channelizer import Channelizer, check_plan, design_taps, factor_rate
from pycusdr_amd.modulator import phase

FS = 1.0e6
TRIPLES = [(2, 3, 7), (3, 5, 3), (16, 25, 401), (31, 64, 100), (24, 25, 24)]


def brute(cz, x, nout_from_zero):
    """Outputs 0 .. nout_from_zero of every channel from the stream x (position 0 first): mix, stuff U - 1 zeros behind every
    sample, convolve with h, keep every D-th."""
    U, D = cz.interp, cz.decim
    n = np.arange(len(x), dtype=np.uint64)
    y = np.empty((cz.K, nout_from_zero), dtype=np.complex128)
    for k, f in enumerate(cz.words):
        with np.errstate(over='ignore'):
            w = np.uint64(0) - n * np.uint64(f)
        z = x.astype(np.complex128) * phase.words_to_iq(w)
        v = np.zeros(len(x) * U, dtype=np.complex128)
        v[::U] = z
        full = np.convolve(v, cz.taps.astype(np.float64))
        y[k] = full[:nout_from_zero * D:D][:nout_from_zero]
    return y


@pytest.mark.parametrize('U,D,T', TRIPLES)
def test_model_is_the_zero_stuffed_convolution(U, D, T):
    rs = np.random.RandomState(U * 100 + D)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    cz = Channelizer(FS, D, h, [123.4e3, 0.0], backend='host', interp=U, max_in=1 << 16)
    out_base, nout = 7 * U + 1, 150                          # not a multiple of U
    assert out_base % U
    in_base, in_count = cz.needed_input(out_base, nout)
    x_all = (rs.standard_normal(in_base + in_count) + 1j * rs.standard_normal(in_base + in_count)).astype(np.complex64)
    want = brute(cz, x_all, out_base + nout)[:, out_base:]
    y, S = cz.model(in_base, x_all[in_base:], out_base, nout)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    assert S.shape == (nout,) and np.all(S > 0)
    # S is the same sum over magnitudes: the brute-force statement on |x| and |h| with freq 0
    v = np.zeros(len(x_all) * U)
    v[::U] = np.abs(x_all.astype(np.complex128))
    want_S = np.convolve(v, np.abs(h.astype(np.float64)))[out_base * D:(out_base + nout) * D:D]
    assert np.abs(S - want_S).max() <= 1e-12 * want_S.max()
    # and from position 0, where the positions below 0 read as zero
    y0, _ = cz.model(0, x_all[:cz.needed_input(0, 40)[1]], 0, 40)
    want0 = brute(cz, x_all, 40)
    assert np.abs(y0 - want0).max() <= 1e-12 * np.abs(want0).max()
    # process() of the host back end is the model, rounded
    got = cz.process(in_base, x_all[in_base:], out_base, nout)
    assert got.dtype == np.complex64 and np.array_equal(got, y.astype(np.complex64))


def todays_model(cz, in_base, x, out_base, out_count):
    """model() as it stood before ``interp`` existed."""
    D, T = cz.decim, cz.T
    x = x.astype(np.complex128)
    first = out_base * D - (T - 1)
    span = (out_count - 1) * D + T
    lo = max(first, 0)
    seg = np.zeros(span, dtype=np.complex128)
    seg[lo - first:] = x[lo - in_base:first + span - in_base]
    n = np.arange(lo, first + span, dtype=np.int64).astype(np.uint64)
    hrev = cz.taps.astype(np.float64)[::-1]
    win = np.lib.stride_tricks.sliding_window_view
    y = np.empty((cz.K, out_count), dtype=np.complex128)
    for k, f in enumerate(cz.words):
        z = seg
        if f != 0:
            with np.errstate(over='ignore'):
                w = np.uint64(0) - n * np.uint64(f)
            z = seg.copy()
            z[lo - first:] = np.where(w == 0, seg[lo - first:], seg[lo - first:] * phase.words_to_iq(w))
        y[k] = win(z, T)[::D] @ hrev
    return y, win(np.abs(seg), T)[::D] @ np.abs(hrev)


@pytest.mark.parametrize('out_base', [0, 1001])
def test_interp_1_is_todays_model_bit_for_bit(out_base):
    rs = np.random.RandomState(5)
    D, T = 5, 23
    h = rs.uniform(-1, 1, T).astype(np.float32)
    a = Channelizer(FS, D, h, [123.4e3, 0.0, -377.7e3], backend='host')
    b = Channelizer(FS, D, h, [123.4e3, 0.0, -377.7e3], backend='host', interp=1)
    assert not a.rational and not b.rational and a.interp == b.interp == 1
    in_base, in_count = a.needed_input(out_base, 200)
    assert (in_base, in_count) == b.needed_input(out_base, 200) == (max(0, out_base * D - (T - 1)), 199 * D + 1 + min(T - 1, out_base * D))
    x = (rs.standard_normal(in_count) + 1j * rs.standard_normal(in_count)).astype(np.complex64)
    ya, Sa = a.model(in_base, x, out_base, 200)
    yb, Sb = b.model(in_base, x, out_base, 200)
    yt, St = todays_model(a, in_base, x, out_base, 200)
    for y, S in ((ya, Sa), (yb, Sb)):
        assert np.array_equal(y.view(np.uint64), yt.view(np.uint64)) and np.array_equal(S.view(np.uint64), St.view(np.uint64))


def test_design_taps():
    for D, kw in ((25, {}), (4, dict(taps_per_phase=3, beta=5.0, cutoff=0.3))):
        assert design_taps(D, interp=1, **kw).tobytes() == design_taps(D, **kw).tobytes()
    h = design_taps(25, interp=16)
    assert h.dtype == np.float32 and len(h) == 25 * 16 + 1 and np.array_equal(h, h[::-1])
    # float32 rounding of 401 taps whose magnitudes sum to sum|h|: at most half an ulp each
    assert abs(h.astype(np.float64).sum() - 16) <= 2.0 ** -24 * np.abs(h).astype(np.float64).sum()
    # the same shape as the integer design, scaled: cutoff / D cycles per virtual sample whatever U
    assert np.allclose(h / 16, design_taps(25), rtol=0, atol=1e-7)
    with pytest.raises(ValueError):
        design_taps(25, interp=0)


@pytest.mark.parametrize('U,D,T', TRIPLES + [(1, 5, 23)])
def test_needed_input_covers_exactly_what_the_model_reads(U, D, T):
    cz = Channelizer(FS, D, np.ones(T, np.float32), [0.0], backend='host', interp=U, max_in=1 << 16)
    for out_base, count in ((0, 1), (0, 9), (1, 1), (U + 1, 2 * U + 3), (1001, 77), ((1 << 40) + 5, 3)):
        reads = set()
        shortest_first = None
        for m in range(out_base, out_base + count):
            q, r = divmod(m * D, U)
            nb = -(-(T - r) // U)
            reads.update(n for n in range(q - nb + 1, q + 1) if n >= 0)
            if m == out_base:
                shortest_first = max(0, q - nb + 1)
        first, n = cz.needed_input(out_base, count)
        assert first + n - 1 == max(reads)                   # the last input is read
        # the first is the uniform bound: the first output's own first tap, or one sample before it for a short branch
        assert first <= min(reads) and first in (shortest_first, max(0, shortest_first - 1))
        assert first >= 0 and n >= 1


def test_check_plan_rejects_what_the_rational_plan_cannot_do():
    taps, words = np.ones(40, np.float32), np.zeros(1, np.uint64)
    check_plan(25, taps, words, 'cf32', 1.0, interp=16)
    check_plan(25, taps, words, 'cf32', 1.0)
    for U, D, t in ((2, 4, taps), (15, 25, taps),            # a common factor
                    (5, 5, taps), (7, 5, taps),              # U >= D
                    (33, 64, taps),                          # U > 32
                    (0, 5, taps),
                    (3, 5, taps[:2])):                       # T < U
        with pytest.raises(ValueError):
            check_plan(D, t, words, 'cf32', 1.0, interp=U)
    with pytest.raises(ValueError):
        Channelizer(FS, 4, taps, [0.0], backend='host', interp=2)


def ratio_of(stages):
    f = Fraction(1)
    for u, d in stages:
        assert 1 <= u <= 32 and 2 <= d <= 64 and u < d and Fraction(u, d).denominator == d
        f *= Fraction(u, d)
    return f


def test_factor_rate():
    assert factor_rate(1.92e6, 153600) == [(2, 25)]
    for fs_in, fs_out, want in ((2.048e6, 76800, Fraction(3, 80)), (1e6, 153600, Fraction(96, 625)), (250e3, 153600, Fraction(384, 625)),
                                (2.4e6, 153600, Fraction(8, 125))):
        st = factor_rate(fs_in, fs_out)
        assert len(st) == 2 and ratio_of(st) == want, st
        assert Fraction(*st[0]) <= Fraction(*st[1])           # the larger reduction first
    assert factor_rate(1e6, 153600) == [(4, 25), (24, 25)]
    assert factor_rate(64, 1) == [(1, 64)] and factor_rate(128, 1) == [(1, 64), (1, 2)]
    assert factor_rate(Fraction(3), Fraction(2)) == [(2, 3)]
    for bad in ((67, 1), (67 * 4, 3), (64, 37), (1, 1), (1, 2)):      # a prime above the limits, no reduction, interpolation
        with pytest.raises(ValueError):
            factor_rate(*bad)


def test_the_entry_point_is_bound_and_exported():
    assert 'mfb_channelizer_set_plan_rational' in _lib.PROTOTYPES
    import __graft_entry__
    import ctypes
    lib = ctypes.CDLL(__graft_entry__.build())
    assert hasattr(lib, 'mfb_channelizer_set_plan_rational')
    assert _lib.load().mfb_abi_version() == 9
