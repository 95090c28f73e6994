"""The channel on the device (mfb_channel_*, csrc/channel_kernels.hpp): against itself under other spans, against the host model
bit for bit where no floating point is involved, within a worked-out bound where it is, and its error codes."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd import channel as ch
from test_channel_host import CHUNKS, _six_frames, _source, check_moments

pytestmark = pytest.mark.gpu

# |device - float64 model| <= C_BOUND * 2^-24 * (gain |src| + sigma max(1, r)) per component.  Twice the worst measured on an MI355X
# over the cases of this file, rounded up -- 3.72, in the sweep of 2^22 noise samples (profiles/channel.md; the six frames gave 2.74
# with noise and 2.31 without, k near 2^24 1.13, the seam 0.93); the ceiling it must stay under is 16: about twice what the roundings add up
# to (~7 units on the noise path: a <= 2 ulp log, a correctly rounded root, mod_phase_to_iq within 4 * 2^-24 and a product; ~10 on
# the rotated signal: four products and two sums on a unit phasor within 4 * 2^-24).
C_BOUND = 8
assert C_BOUND <= 16
U = 2.0 ** -24


def bits(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.uint32)


def pair(seed=0, max_samples=1 << 16, max_source=1 << 12, source=None, fs=1.0e6, max_frames=512):
    dev = ch.Channel(fs, seed=seed, backend='hip', max_samples=max_samples, max_source=max_source, max_frames=max_frames)
    host = ch.Channel(fs, seed=seed, backend='host', max_samples=max_samples, max_source=max_source, max_frames=max_frames)
    if source is not None:
        dev.set_source(source)
        host.set_source(source)
    return dev, host


def measured_c(dev_out, host, base, count, frames, sigma):
    """The worst |device - model| over both components, in units of 2^-24 (gain |src| + sigma max(1, r))."""
    sig, noise, r = host.model_parts(base, count, frames, np.float32(sigma))
    model = sig + noise
    gain_src = np.zeros(count)
    for f in frames:
        lo, hi = max(f.start, base), min(f.start + f.length, base + count)
        if lo < hi:
            gain_src[lo - base:hi - base] = abs(np.float32(f.gain)) * np.abs(host._src[f.src + lo - f.start:f.src + hi - f.start].astype(np.complex128))
    scale = U * (gain_src + float(np.float32(sigma)) * np.maximum(1.0, r))
    d = dev_out.astype(np.complex128) - model
    err = np.maximum(np.abs(d.real), np.abs(d.imag))
    ok = scale > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / scale[ok]).max()) if ok.any() else 0.0


@pytest.fixture(scope='module')
def span():
    """The 5000-sample span with six frames, rendered whole on the device once."""
    dev, host = pair(seed=77, source=_source())
    frames = _six_frames(dev)
    whole = dev.render(0, 5000, frames, sigma=0.25, mute_before=2)
    yield dev, host, frames, whole
    dev.close()


def test_whole_equals_chunks(span):
    dev, _, frames, whole = span
    parts = np.concatenate([dev.render(a, b - a, frames, sigma=0.25, mute_before=2) for a, b in CHUNKS])
    assert np.array_equal(bits(whole), bits(parts))
    assert np.all(whole[:2] == 0) and np.all(whole[2:] != 0)
    adc = (8, 2.0 ** -4)
    a = dev.render(0, 5000, frames, sigma=0.25, adc=adc)
    b = np.concatenate([dev.render(a0, b0 - a0, frames, sigma=0.25, adc=adc) for a0, b0 in CHUNKS])
    assert np.array_equal(bits(a), bits(b))
    q = a.view(np.float32) * 16
    assert np.all(q == np.rint(q)) and q.min() >= -128 and q.max() <= 127 and np.abs(q).max() > 20


@pytest.mark.parametrize('base,count', [(1711, 3000), (1711, 3001), (1, 4999), (258, 1), (4099, 1), (202, 57)])
def test_odd_bases_rerender_the_same_samples(span, base, count):
    """Half pairs at the front (odd base), at the back (odd end), both, and a window that is one half pair."""
    dev, _, frames, whole = span
    again = dev.render(base, count, frames, sigma=0.25, mute_before=2)
    assert np.array_equal(bits(again), bits(whole[base:base + count]))


def test_span_within_the_bound_of_the_model(span):
    dev, host, frames, whole = span
    c = measured_c(whole[2:], host, 2, 4998, frames, 0.25)
    print(f'measured c, six frames with noise: {c:.2f}')
    c0 = measured_c(dev.render(0, 5000, frames), host, 0, 5000, frames, 0.0)
    print(f'measured c, six frames without noise: {c0:.2f}')
    assert max(c, c0) <= C_BOUND


def test_noise_sweep_within_the_bound_of_the_model():
    n = 1 << 22
    dev, host = pair(seed=4, max_samples=n)
    out = dev.render(0, n, sigma=1.0)
    dev.close()
    c = measured_c(out, host, 0, n, [], 1.0)
    print(f'measured c, 2^22 noise samples: {c:.2f}')
    assert c <= C_BOUND


def _placed(src, frames, base, count):
    want = np.zeros(count, dtype=np.complex64)
    for f in frames:
        lo, hi = max(f.start, base), min(f.start + f.length, base + count)
        if lo < hi:
            want[lo - base:hi - base] = src[f.src + lo - f.start:f.src + hi - f.start]
    return want


def test_zero_phase_places_the_source_bit_for_bit():
    src = _source(4096, seed=8)
    src[17] = complex(-0.0, 1e-40)                       # a signed zero and a denormal pass through too
    dev, host = pair(source=src)
    F = lambda start, s, length: dev.frame(start, s, length)      # noqa: E731
    rs = np.random.RandomState(6)
    many, pos = [], 5
    for i in range(300):
        many.append(F(pos, int(rs.randint(0, 4000)), 7))
        pos += 7 + int(rs.randint(0, 4))
    cases = {
        'length 1': ([F(0, 17, 1), F(1, 3, 1), F(2, 4, 1), F(9, 5, 1), F(511, 6, 1), F(512, 7, 1)], 0, 600),
        'touching': ([F(10, 0, 246), F(256, 300, 256), F(512, 17, 513), F(1025, 0, 1)], 0, 1100),
        '300 of 7': (many, 0, pos + 3),
        'clipped in front': ([F(100, 0, 1000)], 613, 700),
        'clipped behind': ([F(100, 0, 1000)], 50, 555),
        'clipped on both sides': ([F(100, 0, 4000)], 1001, 1023),
        'window starts a frame at an odd base': ([F(101, 0, 50)], 101, 60),
    }
    for name, (frames, base, count) in cases.items():
        got = dev.render(base, count, frames)
        assert np.array_equal(bits(got), bits(_placed(src, frames, base, count))), name
        assert np.array_equal(bits(got), bits(host.render(base, count, frames))), name
    dev.close()


@pytest.mark.parametrize('nbits', [8, 16])
def test_adc_ties_and_rails(nbits):
    s = 2.0 ** -5
    top = float((1 << (nbits - 1)) - 1)
    steps = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49, -0.3, top - 0.4, top + 0.5, top + 1, 8 * top, -top - 0.5, -top - 1.5,
                      -8 * top, 3.0], dtype=np.float32)
    want = [0, 0, 2, -2, 2, -2, 0, 0, top, top, top, top, -top - 1, -top - 1, -top - 1, 3]
    src = (steps * np.float32(s)).astype(np.complex64) + 1j * (steps[::-1] * np.float32(s))
    dev, host = pair(source=src)
    fr = [dev.frame(3, 0, len(src))]
    got = dev.render(0, 24, fr, adc=(nbits, s))
    dev.close()
    assert np.array_equal(bits(got), bits(host.render(0, 24, fr, adc=(nbits, s))))
    assert (got.real[3:19] / s).tolist() == want and (got.imag[3:19] / s).tolist() == want[::-1]
    assert not np.signbit(got.view(np.float32)[got.view(np.float32) == 0]).any()


def test_mute_before_inside_a_pair(span):
    dev, _, frames, whole = span
    got = dev.render(0, 64, frames, sigma=0.25, mute_before=7)
    assert np.all(bits(got[:7]) == 0)
    assert np.array_equal(bits(got[7:]), bits(whole[7:64])) and got[7] != 0


def debug_normals(w0, w1):
    lib = _lib.load()
    words = np.ascontiguousarray(np.stack([w0, w1], axis=-1), dtype=np.uint32)
    out = np.zeros(len(words), dtype=np.complex64)
    _lib.check(lib.mfb_debug_channel_normals(0, words.ctypes.data, len(words), out.ctypes.data), 'mfb_debug_channel_normals')
    return out


@pytest.mark.parametrize('base', [(1 << 32) - 3, (1 << 33) - 3])
def test_noise_across_the_32_bit_carries(base):
    """n passes 2^32 (first base) and its block index n >> 1 passes 2^32 (second): the device's words are the model's, and the
    span does not depend on how it is cut."""
    dev, _ = pair(seed=0xFEDCBA9876543210)
    whole = dev.render(base, 4096, sigma=1.0)
    w = ch.noise_words(dev.seed, np.arange(base, base + 4096, dtype=np.uint64))
    assert np.array_equal(bits(whole), bits(debug_normals(w[:, 0], w[:, 1])))
    parts = np.concatenate([dev.render(base + a, b - a, sigma=1.0) for a, b in ((0, 2), (2, 3), (3, 4), (4, 2049), (2049, 4096))])
    dev.close()
    assert np.array_equal(bits(whole), bits(parts))


def test_phase_words_at_large_k():
    """k up to 2^24 - 1 with a rate whose quadratic term wraps 2^64 many times: the last 256 samples against the model's words."""
    n = 1 << 24
    src = np.ones(n, dtype=np.complex64)
    dev, host = pair(max_samples=256, max_source=n, source=src)
    fr = [dev.frame(0, 0, n, 1.0, doppler_hz=-12345.678, rate_hz_per_s=3.3e9, phase_rad=1.0)]
    assert (n * (n - 1) // 2) * fr[0].rate > 1 << 70
    got = dev.render(n - 256, 256, fr)
    dev.close()
    c = measured_c(got, host, n - 256, 256, fr, 0.0)
    print(f'measured c, k near 2^24: {c:.2f}')
    assert c <= C_BOUND and np.abs(np.abs(got) - 1).max() < 1e-6


def test_normals_seam_at_the_ends_of_the_uniform():
    first = np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    second = np.array([0, 1 << 29, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)
    w0, w1 = (a.reshape(-1) for a in np.meshgrid(first, second, indexing='ij'))
    got = debug_normals(w0, w1).reshape(5, 4).astype(np.complex128)
    want = ch.normals_of(w0, w1).reshape(5, 4)
    r = ch.radius_of(w0).reshape(5, 4)
    d = got - want
    c = (np.maximum(np.abs(d.real), np.abs(d.imag)) / (U * np.maximum(1.0, r))).max()
    print(f'measured c, the seam: {c:.2f}')
    assert c <= C_BOUND
    assert np.all(got[3:] == 0)                                  # u = 1: radius 0
    assert np.all(got[:, 0].imag == 0) and np.all(got[:, 2].imag == 0)      # angles 0 and half a turn
    assert np.array_equal(got[0], got[1]) and np.all(got[:3, 0].real > 0) and np.all(got[:3, 2].real < 0)
    assert abs(got[0, 0].real - ch.R_MAX) <= 4 * U * ch.R_MAX and np.abs(got).max() <= 5.77
    assert np.all(np.abs(got[:3, 1].real - got[:3, 1].imag) <= 8 * U * r[:3, 1])          # an eighth of a turn


def test_moments_of_a_million_device_samples():
    n = 1 << 20
    dev, _ = pair(seed=1, max_samples=n)
    x = dev.render(0, n, sigma=1.0).astype(np.complex128)
    dev.close()
    check_moments(x.real, x.imag)


def test_device_source_is_used_in_place_and_windows_stay_on_the_device():
    """A window left on the device is the next render's source: frames of it, placed again, are its samples."""
    src = _source(1024, seed=2)
    dev, _ = pair(source=src)
    first = dev.render(0, 1000, [dev.frame(100, 0, 800)], sigma=0.5)
    ptr, count = dev.render(0, 1000, [dev.frame(100, 0, 800)], sigma=0.5, copy=False, buffer=0)
    assert count == 1000 and ptr % 16 == 0
    dev.set_source(ch.DeviceBatch(ptr, np.array([0, count])))
    again = dev.render(0, 600, [dev.frame(0, 400, 600)], buffer=1)
    dev.close()
    assert np.array_equal(bits(again), bits(first[400:1000]))


def test_misuse_is_an_error_code():
    lib = _lib.load()
    OK, ARG, STATE = _lib.MFB_OK, _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE
    h = C.c_void_p()
    assert lib.mfb_channel_create(None, 0, 64, 64, 4) == ARG
    for bad in ((0, 64, 4), (64, 0, 4), (64, 64, 0)):
        assert lib.mfb_channel_create(C.byref(h), 0, *bad) == ARG and not h
    assert lib.mfb_channel_create(C.byref(h), 0, (1 << 24) + 1, 64, 4) == _lib.MFB_ERR_UNSUPPORTED and not h
    assert lib.mfb_channel_create(C.byref(h), 99, 64, 64, 4) == ARG and not h
    assert lib.mfb_channel_create(C.byref(h), 0, 64, 64, 4) == OK and h
    out = np.zeros(64, dtype=np.complex64)
    ptr, n = C.c_void_p(), C.c_int64()

    def P(**kw):
        return _lib.ChannelParams(**{'base': 0, 'count': 32, 'sigma': 1.0, **kw})

    def frames(*items):
        a = (_lib.ChannelFrame * len(items))()
        for d, (start, src, length, gain) in zip(a, items):
            d.start, d.src, d.length, d.gain = start, src, length, gain
        return a

    def begin(p, fr=None):
        return lib.mfb_channel_begin(h, C.byref(p), fr, 0 if fr is None else len(fr))

    assert lib.mfb_channel_end(h, None) == STATE                                   # _end without _begin
    assert lib.mfb_channel_end(None, None) == ARG and lib.mfb_channel_destroy(None) == ARG
    assert lib.mfb_channel_device_output(h, 0, C.byref(ptr), C.byref(n)) == STATE   # never rendered
    assert lib.mfb_channel_device_output(h, 2, C.byref(ptr), C.byref(n)) == ARG
    assert lib.mfb_channel_device_output(h, 0, None, None) == ARG
    assert lib.mfb_channel_begin(None, C.byref(P()), None, 0) == ARG and lib.mfb_channel_begin(h, None, None, 0) == ARG
    assert lib.mfb_channel_begin(h, C.byref(P()), None, 1) == ARG                   # frames NULL, nframes 1
    assert begin(P(), frames((0, 0, 4, 1.0))) == STATE                              # frames, no source
    assert lib.mfb_channel_set_source(h, None, 8, 0) == ARG
    assert lib.mfb_channel_set_source(h, out.ctypes.data, 0, 0) == ARG
    assert lib.mfb_channel_set_source(h, out.ctypes.data, 65, 0) == ARG             # beyond max_source
    assert lib.mfb_channel_set_source(h, out.ctypes.data, 64, 0) == OK
    for p in (P(count=0), P(count=65), P(base=-1), P(mute_before=-1), P(buffer=2), P(sigma=-1.0), P(sigma=float('nan')),
              P(adc_bits=12, adc_scale=1.0), P(adc_bits=8, adc_scale=3.0), P(adc_bits=16, adc_scale=0.0)):
        assert begin(p) == ARG
    for fr in (frames((0, 0, 0, 1.0)), frames((-1, 0, 4, 1.0)), frames((8, 0, 4, 1.0), (4, 0, 4, 1.0)), frames((0, 0, 8, 1.0), (7, 0, 4, 1.0)),
               frames((0, 61, 4, 1.0)), frames((0, -1, 4, 1.0)), frames((0, 0, 4, float('inf'))),
               frames(*[(i, 0, 1, 1.0) for i in range(5)])):                        # the last: more frames than created for
        assert begin(P(), fr) == ARG
    assert lib.mfb_channel_end(h, None) == STATE                                   # none of them left anything in flight
    assert begin(P(), frames((0, 0, 8, 1.0), (8, 60, 4, 1.0))) == OK
    assert begin(P(buffer=1)) == STATE                                              # _begin while in flight
    assert lib.mfb_channel_set_source(h, out.ctypes.data, 64, 0) == STATE
    assert lib.mfb_channel_device_output(h, 0, C.byref(ptr), C.byref(n)) == STATE
    assert lib.mfb_channel_end(h, out.ctypes.data) == OK
    assert lib.mfb_channel_end(h, None) == STATE
    assert lib.mfb_channel_device_output(h, 0, C.byref(ptr), C.byref(n)) == OK and n.value == 32 and ptr.value
    assert lib.mfb_channel_device_output(h, 1, C.byref(ptr), C.byref(n)) == STATE
    assert np.all(out[:32] != 0) and np.all(out[32:] == 0)
    assert lib.mfb_channel_destroy(h) == OK
    w = np.zeros(2, dtype=np.uint32)
    assert lib.mfb_debug_channel_normals(0, None, 1, out.ctypes.data) == ARG
    assert lib.mfb_debug_channel_normals(0, w.ctypes.data, 0, out.ctypes.data) == ARG
    assert lib.mfb_debug_channel_normals(0, w.ctypes.data, 1, None) == ARG
    with pytest.raises(ValueError):
        ch.LoopbackSource(ch.Channel(1.0, backend='host'), [], 1024, 64, 2, 2)
