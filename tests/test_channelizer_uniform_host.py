"""The uniform polyphase channeliser without a device: ``UniformChannelizer(backend='host')`` is the float64 definition on the exact
raster words, the polyphase identity the device kernel computes (csrc/channelize_uniform_kernels.hpp) is that definition, and the
plan checks mirror the C ABI's."""
from math import gcd

import numpy as np
import pytest

from pycusdr_amd.channelizer import Channelizer, ChannelizerSource, UniformChannelizer, check_plan_uniform, design_taps

FS = 1.024e6             # a rate at which 2 pi (b fs / M) / fs quantises to the exact word for every bin of M = 8 and 16: the comparison
#                          with Channelizer(freqs_hz=...) needs that.  (At 1.0e6 bins 5 and 11 of 16 come out 1024 off: the float
#                          route is no way to name a raster, which is why UniformChannelizer takes integers.)


def noise(rs, n):
    return (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize('M, D, T', [(8, 3, 37), (16, 5, 17)])
def test_model_is_the_channelizers_model_on_the_same_words(M, D, T):
    """All bins of M = 8 and 16, where ``freqs_hz = b fs / M`` quantises to the exact words: 0 difference."""
    rs = np.random.RandomState(M)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    uz = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 12)
    cz = Channelizer(FS, D, h, uz.freqs_hz, backend='host', max_in=1 << 12)
    assert np.array_equal(uz.words, cz.words) and uz.K == cz.K == M
    for out_base in (0, (1 << 40) // D + 3):
        in_base, n = uz.needed_input(out_base, 50)
        x = noise(rs, n)
        ya, Sa = uz.model(in_base, x, out_base, 50)
        yb, Sb = cz.model(in_base, x, out_base, 50)
        assert np.array_equal(ya, yb) and np.array_equal(Sa, Sb)
        assert np.array_equal(uz.process(in_base, x, out_base, 50), cz.process(in_base, x, out_base, 50))


def polyphase(h, M, D, seg, first, out_base, out_count):
    """Branch sums, circular shift, M-point transform, in float64: seg[i] is x[first + i] (zero below position 0)."""
    T = len(h)
    h64 = h.astype(np.float64)
    y = np.empty((M, out_count), dtype=np.complex128)
    for i in range(out_count):
        m = out_base + i
        u = np.zeros(M, dtype=np.complex128)
        for p in range(min(M, T)):
            t = np.arange(p, T, M)
            u[p] = np.sum(h64[t] * seg[m * D - t - first])
        v = u[(np.arange(M) + m * D) % M]
        y[:, i] = np.fft.ifft(v) * M
    return y


@pytest.mark.parametrize('M, D, T, out_base', [(8, 3, 37, 0), (16, 16, 16, 5), (32, 7, 5, 0), (64, 48, 1500, (1 << 40) // 48),
                                               (256, 255, 4096, (1 << 40) // 255)])
def test_polyphase_identity_is_the_definition(M, D, T, out_base):
    rs = np.random.RandomState(T)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    nout = 6
    uz = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 14)
    in_base, n = uz.needed_input(out_base, nout)
    x = noise(rs, n)
    ref, S = uz.model(in_base, x, out_base, nout)
    first = out_base * D - (T - 1)
    seg = np.zeros((nout - 1) * D + T, dtype=np.complex128)
    seg[in_base - first:] = x
    y = polyphase(h, M, D, seg, first, out_base, nout)
    err = np.abs(y - ref).max(axis=0) / S
    print(f'M {M} D {D} T {T}: worst |polyphase - model| / S = {err.max():.2e}')
    assert S.min() > 0 and err.max() <= 1e-12


@pytest.mark.parametrize('M', [64, 256])
def test_words_are_exact(M):
    uz = UniformChannelizer(FS, M, M, [1.0], backend='host')
    assert uz.K == M and list(uz.bins) == list(range(M))
    assert [int(w) for w in uz.words] == [(b << 64) // M for b in range(M)]
    assert uz.words.dtype == np.uint64 and uz.interp == 1 and uz.Tb == uz.T == 1


def test_signed_and_unsigned_indices_name_the_same_channel():
    a = UniformChannelizer(FS, 16, 4, design_taps(4), bins=[-1, -8, 3, -3], backend='host')
    b = UniformChannelizer(FS, 16, 4, design_taps(4), bins=[15, 8, 3, 13], backend='host')
    assert np.array_equal(a.bins, b.bins) and np.array_equal(a.words, b.words)
    assert np.allclose(a.freqs_hz, np.array([-1, -8, 3, -3]) * FS / 16)
    rs = np.random.RandomState(4)
    x = noise(rs, 500)
    assert np.array_equal(a.process(0, x, 0, 100), b.process(0, x, 0, 100))


def test_a_tone_appears_in_its_bin_with_the_taps_gain():
    """x[n] = i^n, a tone at fs / 4 whose samples complex64 holds exactly: at bin b's centre b / M plus the offset f = 1 / 4 - b / M.
    Far from position 0 bin b holds H(f) exp(2 pi i f m D), H(f) = sum_t h[t] exp(-2 pi i f t): gain |H(f)| in every bin: the pass
    band for b = 1 .. 3 of M = 8 at D = 2, the transition band for 0 and 4, the stop band for the others."""
    M, D = 8, 2
    h = design_taps(D)
    T = len(h)
    uz = UniformChannelizer(FS, M, D, h, backend='host', max_in=1 << 12)
    out_base, nout = 100, 64
    in_base, n = uz.needed_input(out_base, nout)
    x = np.array([1, 1j, -1, -1j], dtype=np.complex64)[np.arange(in_base, in_base + n) % 4]
    y, S = uz.model(in_base, x, out_base, nout)
    t = np.arange(T)
    gains = []
    for b in range(M):
        f = 0.25 - b / M
        H = np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * t))
        want = H * np.exp(2j * np.pi * f * (out_base + np.arange(nout)) * D)
        assert np.abs(y[b] - want).max() <= 1e-9, b
        assert np.abs(np.abs(y[b]) - np.abs(H)).max() <= 1e-9, b
        gains.append(np.abs(H))
    # bins 0 and 4 see it 0.25 away, at the foot of the transition band of design_taps(2) (cutoff 0.2); bins 5 .. 7 deep in the stop band
    assert gains[2] > 0.999 and min(gains[1], gains[3]) > 0.99 and max(gains[0], gains[4]) < 0.05 and max(gains[5:]) < 1e-4


def test_check_plan_uniform_raises_for_every_limit():
    ok = dict(nbins=16, decim=4, taps=np.ones(8, np.float32), bins=None, sample_format='cf32', sample_scale=1.0)
    M, D, taps, bins, scale = check_plan_uniform(**ok)
    assert (M, D, scale) == (16, 4, 1.0) and list(bins) == list(range(16)) and bins.dtype == np.int32 and taps.dtype == np.float32
    bad = [dict(nbins=4), dict(nbins=512), dict(nbins=24), dict(decim=1), dict(decim=17), dict(taps=np.ones(0)), dict(taps=np.ones(4097)),
           dict(taps=[1.0, np.nan]), dict(taps=[np.inf]), dict(bins=[]), dict(bins=list(range(16)) + [0]), dict(bins=[16]), dict(bins=[-9]),
           dict(bins=[3, 3]), dict(bins=[-1, 15]), dict(bins=[1.5]), dict(sample_format='sc32'), dict(sample_format='sc16', sample_scale=0.3),
           dict(sample_format='sc8', sample_scale=-0.5), dict(sample_format='sc16', sample_scale=float('inf'))]
    for kw in bad:
        with pytest.raises(ValueError):
            check_plan_uniform(**{**ok, **kw})
    assert check_plan_uniform(**{**ok, 'decim': 16, 'taps': np.ones(4096), 'bins': [-8, 15]})[3].tolist() == [8, 15]
    with pytest.raises(ValueError):
        UniformChannelizer(FS, 8, 4, [1.0], backend='cuda')
    with pytest.raises(ValueError):
        UniformChannelizer(FS, 8, 4, [1.0], backend='host', max_in=(1 << 24) + 1)
    with pytest.raises(ValueError):
        UniformChannelizer(FS, 8, 4, [1.0], backend='host', max_out=(1 << 22) + 1)
    with pytest.raises(ValueError):                           # selected * max_out <= 2^26
        UniformChannelizer(FS, 64, 4, [1.0], backend='host', max_in=1 << 24, max_out=1 << 21)
    UniformChannelizer(FS, 64, 4, [1.0], bins=range(32), backend='host', max_in=1 << 24, max_out=1 << 21)


def test_needed_input_matches_the_channelizers():
    h = design_taps(6)
    uz = UniformChannelizer(FS, 8, 6, h, backend='host')
    cz = Channelizer(FS, 6, h, [0.0], backend='host')
    for out_base, n in ((0, 1), (0, 100), (3, 5), (1000, 77), ((1 << 40) // 6, 9)):
        assert uz.needed_input(out_base, n) == cz.needed_input(out_base, n)
    with pytest.raises(ValueError):
        uz.needed_input(-1, 1)


def test_a_source_takes_it_and_refuses_the_host_back_end_when_iterated():
    uz = UniformChannelizer(FS, 8, 4, design_taps(4), bins=[2, 6], backend='host', max_in=1 << 14, max_out=1 << 12)
    src = ChannelizerSource(uz, 1, None, 1024, 128, 2, 3)
    assert len(src) == 3 and src.window_input(1) == uz.needed_input(src.window_base(1), src.count)
    with pytest.raises(ValueError, match="not 'hip'"):
        next(iter(src))
    with pytest.raises(ValueError):
        ChannelizerSource(uz, 2, None, 1024, 128, 2, 3)


def test_decimation_need_not_divide_the_bins():
    assert gcd(7, 32) == 1
    UniformChannelizer(FS, 32, 7, design_taps(7), backend='host')
