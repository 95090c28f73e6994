"""The channeliser's host model (``Channelizer(backend='host')``, the float64 yardstick of the device), its plan arithmetic, the
tap design and the window bases of ``ChannelizerSource``.  No GPU."""
import numpy as np
import pytest

from pycusdr_amd.channel import signed_quantise
from pycusdr_amd.channelizer import Channelizer, ChannelizerSource, check_plan, design_taps

FS = 1.0e6
MASK = (1 << 64) - 1


def direct(x, in_base, h, D, word, out_base, out_count):
    """The definition, one output and one tap at a time, Python integers for the phase."""
    y = np.zeros(out_count, dtype=np.complex128)
    for j in range(out_count):
        m = out_base + j
        acc = 0j
        for t in range(len(h)):
            n = m * D - t
            if n < 0:
                continue
            phi = (n * int(word)) & MASK
            acc += float(h[t]) * complex(x[n - in_base]) * np.exp(-2j * np.pi * (phi / 2.0 ** 64))
        y[j] = acc
    return y


def make(decim, taps, freqs, **kw):
    return Channelizer(FS, decim, taps, freqs, backend='host', **kw)


@pytest.mark.parametrize('D', [2, 3, 16])
@pytest.mark.parametrize('base', [0, (1 << 40) + 3])
def test_host_model_equals_the_direct_double_loop(D, base):
    rs = np.random.RandomState(D)
    for T in (1, D - 1, D, D + 1, 4 * D + 3):
        if T < 1:
            continue
        h = rs.uniform(-1, 1, T).astype(np.float32)
        freqs = [0.0, 123456.789, -FS / 2 + 1.0]
        cz = make(D, h, freqs)
        nout = 9
        in_base, in_count = cz.needed_input(base, nout)
        x = (rs.standard_normal(in_count) + 1j * rs.standard_normal(in_count)).astype(np.complex64)
        y, S = cz.model(in_base, x, base, nout)
        for k in range(3):
            ref = direct(x, in_base, cz.taps, D, cz.words[k], base, nout)
            # the direct loop's phase is one float64 division of the word: 2^-53 turns, far below this
            assert np.abs(y[k] - ref).max() <= 1e-11 * max(1.0, S.max()), (D, T, base, k)
        assert np.array_equal(cz.process(in_base, x, base, nout), y.astype(np.complex64))
    # the words of the large base wrapped: n * freq exceeds 2^64 many times over
    if base:
        assert base * D * int(cz.words[1]) > 1 << 64


def test_host_model_is_chunk_invariant():
    rs = np.random.RandomState(5)
    D, T = 5, 23
    cz = make(D, rs.uniform(-1, 1, T).astype(np.float32), [50e3, -200e3, 0.0])
    base, nout = 1000, 64
    in_base, in_count = cz.needed_input(base, nout)
    x = (rs.standard_normal(in_count + 20) + 1j * rs.standard_normal(in_count + 20)).astype(np.complex64)
    whole = cz.process(in_base, x[:in_count], base, nout)
    at, parts = base, []
    for n in (1, 7, 30, 26):
        b, c = cz.needed_input(at, n)
        parts.append(cz.process(b, x[b - in_base:b - in_base + c], at, n))
        at += n
    assert np.array_equal(np.concatenate(parts, axis=1).view(np.uint32), whole.view(np.uint32))
    # a wider input window changes nothing
    assert np.array_equal(cz.process(in_base, x, base, nout).view(np.uint32), whole.view(np.uint32))


def test_identity_plan_passes_every_decim_th_sample():
    rs = np.random.RandomState(6)
    x = (rs.standard_normal(100) + 1j * rs.standard_normal(100)).astype(np.complex64)
    for D in (2, 5, 64):
        cz = make(D, [1.0], [0.0])
        n = (len(x) - 1) // D + 1
        assert np.array_equal(cz.process(0, x, 0, n)[0].view(np.uint32), np.ascontiguousarray(x[::D][:n]).view(np.uint32))


def test_integer_formats_are_scaled_integers():
    rs = np.random.RandomState(7)
    raw = rs.randint(-32768, 32768, (64, 2)).astype(np.int16)
    cz = make(2, [1.0], [0.0], sample_format='sc16', sample_scale=2.0 ** -15)
    f = raw.astype(np.float32) * np.float32(2.0 ** -15)
    assert np.array_equal(cz.process(0, raw, 0, 32)[0], (f[::2, 0] + 1j * f[::2, 1]).astype(np.complex64))


def test_needed_input_arithmetic():
    cz = make(4, np.ones(9, dtype=np.float32), [0.0])
    assert cz.needed_input(0, 1) == (0, 1)                  # inputs -8 .. 0, clipped at 0
    assert cz.needed_input(0, 3) == (0, 9)                  # .. 8
    assert cz.needed_input(2, 1) == (0, 9)                  # 0 .. 8: exactly at the edge
    assert cz.needed_input(3, 2) == (4, 13)                 # 4 .. 16
    assert cz.needed_input(1 << 40, 5) == ((4 << 40) - 8, 8 + 16 + 1)
    with pytest.raises(ValueError):
        cz.needed_input(-1, 1)
    with pytest.raises(ValueError):
        cz.needed_input(0, 0)
    x = np.zeros(13, dtype=np.complex64)
    cz.process(4, x, 3, 2)
    for in_base, n in ((5, 12), (4, 12)):                   # one sample short at either end
        with pytest.raises(ValueError):
            cz.process(in_base, x[:n], 3, 2)


def test_design_taps():
    for D, tpp in ((4, 16), (16, 16), (3, 14)):
        h = design_taps(D, tpp)
        T = D * tpp + 1
        assert h.dtype == np.float32 and len(h) == T
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(h, h[::-1])
        H = np.abs(np.fft.rfft(h.astype(np.float64), 1 << 16))
        f = np.arange(len(H)) / float(1 << 16)                # cycles per input sample
        stop = f >= (1.0 - 0.4) / D
        att = -20 * np.log10(H[stop].max())
        # a Kaiser window with beta = 8 has side lobes near -80 dB (Kaiser's A = 8.7 + beta / 0.1102); its transition band is
        # (A - 8) / (2.285 * 2 pi * (T - 1)) cycles wide, centred on the cutoff: 0.318 / (decim * taps_per_phase) to either side,
        # which ends before (1 - cutoff) / decim, where the alias zone begins, from 13 taps per phase on
        assert att > 70.0, (D, tpp, att)
        assert abs(20 * np.log10(H[np.searchsorted(f, 0.4 / D)]) + 6.0) < 0.5     # the cutoff is the -6 dB point
    assert len(design_taps(4)) == 65


def test_plan_validation():
    ok = dict(decim=4, taps=np.ones(5, dtype=np.float32), words=np.zeros(2, dtype=np.uint64), sample_format='cf32', sample_scale=1.0)
    check_plan(**ok)
    for bad in (dict(decim=1), dict(decim=65), dict(taps=np.ones(0)), dict(taps=np.ones(1025)), dict(taps=[1.0, np.nan]),
                dict(taps=[np.inf]), dict(words=np.zeros(0, dtype=np.uint64)), dict(words=np.zeros(17, dtype=np.uint64)),
                dict(sample_format='sc32'), dict(sample_format='sc16', sample_scale=0.3), dict(sample_format='sc8', sample_scale=-0.5),
                dict(sample_format='sc8', sample_scale=0.0)):
        with pytest.raises(ValueError):
            check_plan(**{**ok, **bad})
    check_plan(**{**ok, 'sample_format': 'sc16', 'sample_scale': 2.0 ** -11})
    with pytest.raises(ValueError):
        make(4, [1.0], [FS])                                # beyond fs / 2
    with pytest.raises(ValueError):
        Channelizer(FS, 4, [1.0], [0.0], backend='cuda')
    with pytest.raises(ValueError):
        make(4, [1.0], [0.0], max_in=(1 << 24) + 1)
    cz = make(4, [1.0], [-FS / 4, FS / 4])
    assert int(cz.words[0]) == 3 << 62 and int(cz.words[1]) == 1 << 62        # a negative frequency is the two's complement
    assert np.array_equal(cz.words, signed_quantise(2 * np.pi * np.array([-0.25, 0.25])))
    with pytest.raises(ValueError):
        cz.process(0, (1234, 8), 0, 1)                      # device memory on the host back end


def test_channelizer_source_window_bases():
    N, ov, B = 1024, 128, 3
    cz = make(4, design_taps(4), [0.0, 1.0e5], max_in=1 << 15)
    src = ChannelizerSource(cz, 1, None, N, ov, B, 4)
    stride = N - ov
    assert src.count == B * stride + ov and len(src) == 4
    for w in range(4):
        assert src.window_base(w) == w * B * stride
        first = max(0, src.window_base(w) * 4 - 64)
        assert src.window_input(w) == (first, (src.window_base(w) + src.count - 1) * 4 - first + 1)
    # consecutive windows share exactly the overlap
    assert src.window_base(1) + ov - (src.window_base(0) + src.count) == 0
    with pytest.raises(ValueError):
        ChannelizerSource(cz, 2, None, N, ov, B, 4)
    with pytest.raises(ValueError):
        ChannelizerSource(cz, 0, None, 1 << 16, ov, B, 4)   # more than max_in / max_out
    with pytest.raises(ValueError):
        next(iter(src))                                     # the host back end yields no device windows
