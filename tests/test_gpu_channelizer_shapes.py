"""The channeliser's kernel (pycusdr_amd/csrc/channelize_kernels.hpp) at the shapes tests/test_gpu_channelizer.py leaves out: the
128-lane workgroup, the decimations at which the staging's fp32 estimate of p / D is corrected (41, 47, 55, 61), tap counts
around the unroll of 8, every size of channel group of either kind (4, 2, 1; tuned and zero-frequency) with the zero-frequency
channels scattered among the others, any cut of a span at the two narrower tiles, and a handle larger than its plan, re-planned.
tests/test_edge_shapes_host.py proves that the shapes of tests/edge_shapes.py have the tile and the correction they are listed
for.  The yardstick is ``Channelizer.model`` (float64) throughout.

The error bound is that of test_gpu_channelizer.py: per component |device - model| <= c * 2^-24 * S_m, S_m = sum_t |h[t]| |x[m D - t]|,
with the derived ceiling c <= 3 T + 24 (2.83 T for the sequential fp32 sum of 2 T products per component, less than 24 for the
two phasors, the tap's rounding and the rotation).  C_BOUND pins twice the worst c measured over this file's cases on an MI355X
(profiles/channelizer.md has the figure per T)."""
import ctypes as C

import numpy as np
import pytest

import edge_shapes as es
from pycusdr_amd import _lib
from pycusdr_amd.channelizer import Channelizer

pytestmark = pytest.mark.gpu

FS = 1.0e6
EPS = 2.0 ** -24
C_BOUND = 8                       # twice the worst measured c (3.58: D = 5, T = 23, 6 tuned and 7 zero-frequency channels), rounded up
assert C_BOUND <= 3 * min(T for _, T, _, _ in es.CHZ_SHAPES) + 24
WORST = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def noise(rs, n, fmt):
    """0.3 sigma noise in the plan's sample format: complex64, or integers below full scale"""
    x = 0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    if fmt == 'cf32':
        return x.astype(np.complex64)
    full = 32767 if fmt == 'sc16' else 127
    q = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) * full), -full - 1, full)
    return q.astype(np.int16 if fmt == 'sc16' else np.int8)


def scale_of(fmt):
    return {'cf32': 1.0, 'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}[fmt]


def taps_of(rs, T):
    return (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)


def worst_c(cz, T, y, in_base, x, out_base, nout):
    """max over channels, outputs and components of |y - model| / (2^-24 S); S > 0 everywhere, nothing is masked"""
    ref, S = cz.model(in_base, x, out_base, nout)
    assert np.all(S > 0) and np.abs(ref).max() > 0
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    c = float((err / (EPS * S)).max())
    WORST[T] = max(WORST.get(T, 0.0), c)
    return c


BOUND_CASES = [(D, T, tile, fmt, large) for D, T, tile, _ in es.CHZ_SHAPES for fmt in es.CHZ_BOUND_FORMATS.get((D, T), ('cf32',))
               for large in (False, True)]


@pytest.mark.parametrize('D,T,tile,fmt,large', BOUND_CASES)
def test_shapes_within_the_bound_of_the_model(D, T, tile, fmt, large):
    rs = np.random.RandomState(1000 * D + T)
    h = taps_of(rs, T)
    freqs = [151.7e3, 0.0, -288.8e3, 0.49999993 * FS, 37.3e3]          # a group of four and one zero-frequency channel
    nout = 2 * tile + 5
    out_base = ((1 << 40) // D + 3) if large else 0
    cz = Channelizer(FS, D, h, freqs, sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 15)
    try:
        assert cz.info() == (tile, T)
        in_base, in_count = cz.needed_input(out_base, nout)
        x = noise(rs, in_count, fmt)
        y = cz.process(in_base, x, out_base, nout)
        c = worst_c(cz, T, y, in_base, x, out_base, nout)
    finally:
        cz.close()
    print(f'D {D} T {T} tile {tile} {fmt} out_base {out_base}: worst c = {c:.2f} (ceiling {3 * T + 24}); '
          f'worst per T so far {dict(sorted(WORST.items()))}')
    assert c <= 3 * T + 24
    assert c <= C_BOUND


# ---- channel counts ----
FREQ_POOL = [(-1) ** i * (30.0e3 + 27.1e3 * i) for i in range(16)]   # distinct, both signs, |f| < fs / 2
_SHARED = {}


def shared(D, T):
    """Per shape, made once and left unchanged: taps, the span, its input, and the K = 1 output of every frequency asked for."""
    if (D, T) not in _SHARED:
        rs = np.random.RandomState(77 * D + T)
        h = taps_of(rs, T)
        tile = es.chz_threads(D, T)
        nout, out_base = 2 * tile + 5, 1001
        probe = Channelizer(FS, D, h, [0.0], backend='host')
        in_base, in_count = probe.needed_input(out_base, nout)
        x = noise(rs, in_count, 'cf32')
        x.setflags(write=False)
        _SHARED[D, T] = dict(h=h, tile=tile, nout=nout, out_base=out_base, in_base=in_base, x=x, single={})
    return _SHARED[D, T]


def single(D, T, f):
    s = shared(D, T)
    if f not in s['single']:
        one = Channelizer(FS, D, s['h'], [f], max_in=1 << 15)
        try:
            y = one.process(s['in_base'], s['x'], s['out_base'], s['nout'])[0]
        finally:
            one.close()
        y.setflags(write=False)
        s['single'][f] = y
    return s['single'][f]


@pytest.mark.parametrize('ncplx,nreal', es.CHZ_COUNTS)
@pytest.mark.parametrize('D,T', es.CHZ_COUNT_SHAPES)
def test_channel_counts(D, T, ncplx, nreal):
    """Every group size of either kind, the zero-frequency channels scattered among the tuned ones: every channel within the
    bound of the model, and bit-identical to the K = 1 plan of its own frequency on the same input."""
    s = shared(D, T)
    real = es.scatter_real(ncplx, nreal, es.CHZ_COUNTS.index((ncplx, nreal)))
    K = ncplx + nreal
    rot = (3 * ncplx) % 5                                     # a frequency does not sit at the same place of a group in every plan
    pool = iter(FREQ_POOL[rot:] + FREQ_POOL[:rot])
    freqs = [0.0 if real[k] else next(pool) for k in range(K)]
    assert sum(f == 0.0 for f in freqs) == nreal and len({f for f in freqs if f}) == ncplx
    if ncplx >= 2:
        assert {f > 0 for f in freqs if f} == {True, False}
    cz = Channelizer(FS, D, s['h'], freqs, max_in=1 << 15)
    try:
        assert cz.info()[0] == s['tile'] and int((cz.words != 0).sum()) == ncplx
        # the output set first takes another input's results: a channel the kernel left unwritten shows those, not whatever an
        # earlier handle left in the same memory (every zero-frequency channel of every plan here has the same samples)
        cz.process(s['in_base'], s['x'][::-1], s['out_base'], s['nout'], buffer=0)
        y = cz.process(s['in_base'], s['x'], s['out_base'], s['nout'], buffer=0)
        c = worst_c(cz, T, y, s['in_base'], s['x'], s['out_base'], s['nout'])
    finally:
        cz.close()
    print(f'D {D} T {T} ncplx {ncplx} nreal {nreal} zero-frequency at {np.flatnonzero(real).tolist()}: worst c = {c:.2f}; '
          f'worst per T so far {dict(sorted(WORST.items()))}')
    assert c <= 3 * T + 24
    assert c <= C_BOUND
    for k, f in enumerate(freqs):
        assert np.array_equal(bits(y[k]), bits(single(D, T, f))), (k, f)


# ---- any cut of a span ----
@pytest.mark.parametrize('D,T,fmt', es.CHZ_CUT_SHAPES)
def test_any_cut_at_the_narrower_tiles(D, T, fmt):
    """test_pure_function_of_position's chunking at the 128-lane and the 64-lane tile: a span computed whole equals the same span
    in uneven chunks, from input windows of either parity of in_base, into either output set, bit for bit."""
    rs = np.random.RandomState(31 * D + T)
    h = taps_of(rs, T)
    cz = Channelizer(FS, D, h, [123.4e3, 0.0, -377.7e3], sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 16)
    try:
        tile = cz.info()[0]
        assert tile == es.chz_threads(D, T) and tile < 256
        counts = (1, tile - 1, tile, tile + 1, 2 * tile + 7, 3)
        base, nout = 1001, sum(counts)
        in_base, in_count = cz.needed_input(base, nout)
        x = noise(rs, in_count, fmt)
        whole = cz.process(in_base, x, base, nout)
        c = worst_c(cz, T, whole, in_base, x, base, nout)
        print(f'D {D} T {T} tile {tile} {fmt}: worst c = {c:.2f}; worst per T so far {dict(sorted(WORST.items()))}')
        assert c <= C_BOUND
        parities, sets, at = set(), set(), base
        for i, n in enumerate(counts):
            b, cnt = cz.needed_input(at, n)
            if i % 3 == 2 and b > in_base:                   # a wider window than needed, from one sample earlier
                b, cnt = b - 1, cnt + 1
            parities.add(b & 1)
            sets.add(i & 1)
            part = cz.process(b, x[b - in_base:b - in_base + cnt], at, n, buffer=i & 1)
            assert np.array_equal(bits(part), bits(whole[:, at - base:at - base + n])), (i, n)
            at += n
        assert at == base + nout and parities == {0, 1} and sets == {0, 1}
    finally:
        cz.close()


# ---- a handle larger than its plan, re-planned ----
def test_roomy_handle_replanned():
    """tap_stride is the handle's capacity, not the plan's T: plan A in a handle for 16 channels of 1024 taps, then the identity
    plan B, then A again.  A's two results equal each other and an exact-fit handle's, bit for bit; B's is the identity."""
    lib = _lib.load()
    R = es.CHZ_ROOMY
    (DA, TA, KA), (DB, TB, KB) = R['A'], R['B']
    rs = np.random.RandomState(41)
    fit = Channelizer(FS, DA, taps_of(rs, TA), [211.1e3, 0.0, -97.3e3, 412.9e3, -333.3e3][:KA], max_in=R['max_in'])
    h = C.c_void_p()
    try:
        nout, out_base = 2 * fit.info()[0] + 5, 1001
        in_base, in_count = fit.needed_input(out_base, nout)
        x = noise(rs, R['max_in'], 'cf32')
        want = fit.process(in_base, x[:in_count], out_base, nout)
        assert fit.info() == (128, TA)
        assert lib.mfb_channelizer_create(C.byref(h), 0, R['max_channels'], R['max_taps'], R['max_in'], R['max_out']) == _lib.MFB_OK

        def plan(D, taps, words):
            assert lib.mfb_channelizer_set_plan(h, D, taps.ctypes.data, len(taps), words.ctypes.data, len(words), 0, 1.0) == _lib.MFB_OK

        def run(in_base, in_count, out_base, nout, K):
            P = _lib.ChannelizerParams(in_base=in_base, out_base=out_base, in_count=in_count, out_count=nout, input=0, buffer=0)
            assert lib.mfb_channelizer_begin(h, C.byref(P)) == _lib.MFB_OK
            y = np.empty((K, nout), np.complex64)
            assert lib.mfb_channelizer_end(h, y.ctypes.data) == _lib.MFB_OK
            return y

        plan(DA, fit.taps, fit.words)
        tile, cap = C.c_int(), C.c_int()
        assert lib.mfb_channelizer_info(h, C.byref(tile), C.byref(cap)) == _lib.MFB_OK and (tile.value, cap.value) == (128, R['max_taps'])
        host, nbytes = C.c_void_p(), C.c_size_t()
        assert lib.mfb_channelizer_input_buffer(h, 0, C.byref(host), C.byref(nbytes)) == _lib.MFB_OK and nbytes.value == 8 * R['max_in']
        pinned = np.frombuffer((C.c_uint8 * nbytes.value).from_address(host.value), dtype=np.complex64)
        pinned[:] = x                                        # position in_base of plan A's stream, position 0 of plan B's
        a1 = run(in_base, in_count, out_base, nout, KA)
        plan(DB, np.ones(TB, np.float32), np.zeros(KB, np.uint64))
        assert lib.mfb_channelizer_info(h, C.byref(tile), C.byref(cap)) == _lib.MFB_OK and tile.value == 256
        b = run(0, DB * (R['max_out'] - 1) + 1, 0, R['max_out'], KB)
        plan(DA, fit.taps, fit.words)
        a2 = run(in_base, in_count, out_base, nout, KA)
        assert np.array_equal(bits(b[0]), bits(x[:DB * R['max_out']:DB]))
        assert np.array_equal(bits(a1), bits(a2))
        assert np.array_equal(bits(a1), bits(want))
        c = worst_c(fit, TA, a1, in_base, x[:in_count], out_base, nout)
        print(f'roomy handle, D {DA} T {TA} K {KA}: worst c = {c:.2f}; worst per T so far {dict(sorted(WORST.items()))}')
        assert c <= C_BOUND
    finally:
        if h:
            assert lib.mfb_channelizer_destroy(h) == _lib.MFB_OK
        fit.close()
