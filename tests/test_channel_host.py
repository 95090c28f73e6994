"""The channel's host model (pycusdr_amd/channel.py, backend='host'): the integers the device shares with it -- Philox words, the
uniform, the phase words -- and the rules around them.  No GPU."""
import numpy as np
import pytest

from pycusdr_amd import channel as ch
from pycusdr_amd import signals
from pycusdr_amd.modulator import phase

CHUNKS = ((0, 1), (1, 258), (258, 4099), (4099, 5000))


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


def test_philox_known_answers():
    """The three known answers of Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert _hex(ch.philox4x32([0, 0, 0, 0], [0, 0])) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert _hex(ch.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert _hex(ch.philox4x32([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_noise_words_pair_up():
    """Samples 2p and 2p + 1 take the halves of block p; the counter carries into its second word at n = 2**33."""
    seed = 0x0123456789ABCDEF
    n = np.array([0, 1, 6, 7, (1 << 33) - 1, 1 << 33, (1 << 33) + 1], dtype=np.uint64)
    w = ch.noise_words(seed, n)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for i, p in enumerate((0, 0, 3, 3, (1 << 32) - 1, 1 << 32, 1 << 32)):
        block = ch.philox4x32([p & 0xFFFFFFFF, p >> 32, 0, 0], key)
        assert np.array_equal(w[i], block[2 * (int(n[i]) & 1):][:2])


def test_uniform_ends():
    u = ch.uniform_of(np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64))
    assert u[0] == u[1] == 2.0 ** -24 and u[2] == 2.0 ** -23 and u[3] == u[4] == 1.0
    assert np.all(np.float32(u) == u)                               # exact in fp32
    r = ch.radius_of(np.array([0, 0xFFFFFFFF], dtype=np.uint64))
    assert r[1] == 0.0 and abs(r[0] - ch.R_MAX) < 1e-12 and 5.76 < ch.R_MAX < 5.77


@pytest.mark.parametrize('rate_rad', [3.1e-9, -3.1e-9, 0.0])
def test_phase_polynomial_is_the_running_sum(rate_rad):
    """phi(k) = phase0 + k freq + (k (k - 1) / 2) rate against a running uint64 sum of a frequency that itself advances by rate."""
    p0, fq, rt = (int(ch.signed_quantise(v)) for v in (0.7, -0.0123, rate_rad))
    if rate_rad < 0:
        assert rt == (1 << 64) - int(phase.quantise(-rate_rad))    # two's complement of the magnitude
    M = (1 << 64) - 1
    want, ph, f = [], p0, fq
    for _ in range(5000):
        want.append(ph)
        ph = (ph + f) & M
        f = (f + rt) & M
    got = ch.phase_words(p0, fq, rt, np.arange(5000, dtype=np.uint64))
    assert np.array_equal(got, np.array(want, dtype=np.uint64))


def _six_frames(c):
    return [c.frame(3, 0, 200, 0.5, 1200.0, 4.0e5, 0.3), c.frame(203, 10, 55, 1.0, -800.0, -2.5e5), c.frame(258, 0, 3, 2.0),
            c.frame(1000, 100, 1500, 1.0, 50.0, 1.0e6, -1.0), c.frame(4090, 40, 20, 1.5, -3000.0), c.frame(4800, 0, 400, 1.0, 10.0, -9.0e5)]


def _source(n=2048, seed=5):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n) + 1j * rs.standard_normal(n)).astype(np.complex64)


def test_host_render_is_chunk_invariant():
    c = ch.Channel(1.0e6, seed=77, backend='host', max_samples=5000)
    c.set_source(_source())
    frames = _six_frames(c)
    for adc in (None, (8, 2.0 ** -4)):
        whole = c.render(0, 5000, frames, sigma=0.25, mute_before=2, adc=adc)
        parts = np.concatenate([c.render(a, b - a, frames, sigma=0.25, mute_before=2, adc=adc) for a, b in CHUNKS])
        assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
        assert np.all(whole[:2] == 0) and (adc or np.all(whole[2:] != 0))


def test_zero_phase_unit_gain_passes_the_source_through():
    c = ch.Channel(1.0e6, backend='host', max_samples=512)
    src = _source(300)
    c.set_source(src)
    out = c.render(10, 400, [c.frame(20, 5, 100), c.frame(120, 0, 300)])
    want = np.zeros(400, dtype=np.complex64)
    want[10:110] = src[5:105]
    want[110:400] = src[:290]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_sigma_for_is_awgns_bookkeeping():
    """signals.awgn adds sqrt(noiseP / 2) * (randn + i randn) with noiseP = 10^(-(snr - sigp) / 10): recovered from its output."""
    rs = np.random.RandomState(3)
    sig = 0.7 * np.exp(1j * rs.uniform(0, 6.28, 4096))
    power = np.linalg.norm(np.abs(sig), 2) ** 2 / len(sig)
    for snr, measured in ((15.0, True), (3.0, True), (-2.0, False)):
        noisy = signals.awgn(sig, snr, measured=measured, rng=np.random.RandomState(9))
        r = np.random.RandomState(9)
        unit = r.randn(len(sig)) + 1j * r.randn(len(sig))
        sigma = np.median(np.abs(noisy - sig) / np.abs(unit))
        assert abs(ch.Channel.sigma_for(snr, power, measured) / sigma - 1) < 1e-9


def test_adc_rule_ties_and_rails():
    s = 2.0 ** -3
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49, -0.3, 126.6, 127.5, 1000.0, -127.5, -128.5, -1000.0], dtype=np.float32) * s
    q = ch.adc_quantise(x, 8, s) / s
    assert q.tolist() == [0, 0, 2, -2, 2, -2, 0, 0, 127, 127, 127, -128, -128, -128]
    assert not np.signbit(q).any() or np.all(q[np.signbit(q)] < 0)          # no -0: the integers have none
    q = ch.adc_quantise(np.array([32766.5, 32767.5, 1e9, -32768.5, -1e9], dtype=np.float32), 16, 1.0)
    assert q.tolist() == [32766, 32767, 32767, -32768, -32768]
    c = ch.Channel(1.0, backend='host', max_samples=8)
    for bad in ((12, 1.0), (8, 3.0), (16, 0.0), (16, -1.0)):
        with pytest.raises(ValueError):
            c.render(0, 4, adc=bad)


def test_frame_checks_raise():
    c = ch.Channel(1.0e6, backend='host', max_samples=1000, max_source=100, max_frames=2)
    with pytest.raises(ValueError):
        c.render(0, 10, [ch.Frame(0, 0, 5, 1.0, 0, 0, 0)])                  # no source
    c.set_source(np.ones(100, dtype=np.complex64))
    F = lambda start, src, length, gain=1.0: ch.Frame(start, src, length, gain, 0, 0, 0)      # noqa: E731
    for frames in ([F(0, 0, 0)], [F(-1, 0, 5)], [F(10, 0, 5), F(5, 0, 5)], [F(0, 0, 10), F(9, 0, 5)], [F(0, 96, 5)], [F(0, -1, 5)],
                   [F(0, 0, 5, float('nan'))], [F(0, 0, 1), F(1, 0, 1), F(2, 0, 1)]):
        with pytest.raises(ValueError):
            c.render(0, 10, frames)
    for kw in (dict(base=-1, count=10), dict(base=0, count=0), dict(base=0, count=1001), dict(base=0, count=10, sigma=-1.0),
               dict(base=0, count=10, sigma=float('inf')), dict(base=0, count=10, mute_before=-1)):
        with pytest.raises(ValueError):
            c.render(frames=[], **{'sigma': 0.0, **kw})
    with pytest.raises(ValueError):
        c.set_source(np.ones(101, dtype=np.complex64))
    with pytest.raises(ValueError):
        ch.Channel(1.0, backend='cuda')
    assert len(c.render(0, 10, [F(0, 0, 10), F(10, 95, 5)])) == 10          # touching frames, the source's last sample: fine


def test_moments_of_a_million_samples():
    """2^20 samples of seed 1, sigma 1.  Each bound is six standard errors of its estimator at n = 2^20.  The model's own values:
    mean -9.5e-4 / -5.4e-4 (bound 5.9e-3), var - 1 = 5.0e-4 / 1.4e-3 (8.3e-3), corr 1.1e-3 (5.9e-3), excess kurtosis 4.9e-3 / -6.4e-3
    (2.9e-2; the tail cut at 5.77 sigma removes 1e-6 of it)."""
    n = 1 << 20
    c = ch.Channel(1.0e6, seed=1, backend='host', max_samples=n)
    x = c.render(0, n, sigma=1.0).astype(np.complex128)
    check_moments(x.real, x.imag)


def check_moments(i, q):
    n = len(i)
    for v in (i, q):
        assert abs(v.mean()) <= 6 / np.sqrt(n)
        assert abs(v.var() - 1) <= 6 * np.sqrt(2 / n)
        assert abs(((v - v.mean()) ** 4).mean() / v.var() ** 2 - 3) <= 6 * np.sqrt(24 / n)
    assert abs(np.corrcoef(i, q)[0, 1]) <= 6 / np.sqrt(n)
