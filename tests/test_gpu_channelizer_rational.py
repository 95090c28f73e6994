"""Rational resampling in the device channeliser (csrc/channelize_rational_kernels.hpp, mfb_channelizer_set_plan_rational) against
its contract: exact where nothing rounds, the integer kernel's bits at U = 1, a pure function of the absolute position bit for
bit, within a derived bound of the float64 model, zeros below position 0, an error code for every misuse, two stages chained on
device pointers.

The error bound.  Per component |device - model| <= c * 2^-24 * S_m with S_m = sum_j |h[r + jU]| |x[q - j]|.  The derivation is
that of tests/test_gpu_channelizer.py with the Tb = ceil(T / U) terms a branch has in place of T: a sequential fp32 sum of 2 Tb
products per component over terms bounded by sqrt(2) S gives 2.83 Tb; the tap phasor and the rotation phasor, each within
4 * 2^-24 per component, the tap's rounding and the rotation's products and sum add less than 24: c <= 3 Tb + 24.  Derived, not
measured, so it is fixed here.  profiles/channelizer_rational.md has the worst measured c per case; C_BOUND pins twice the worst
of them, rounded up."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd.channelizer import Channelizer, design_taps, factor_rate

pytestmark = pytest.mark.gpu

FS = 1.0e6
EPS = 2.0 ** -24
C_BOUND = 13                      # twice the worst measured c, rounded up: 6.08, (U, D, T) = (16, 25, 401), noise, on one MI355X
                                  # (profiles/channelizer_rational.md has every case)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def quantise(x, fmt):
    if fmt == 'cf32':
        return x.astype(np.complex64)
    full = 32767 if fmt == 'sc16' else 127
    q = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) * full), -full - 1, full)
    return q.astype(np.int16 if fmt == 'sc16' else np.int8)


def noise(rs, n, fmt='cf32'):
    return quantise(0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n)), fmt)


def scale_of(fmt):
    return {'cf32': 1.0, 'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}[fmt]


def to_c64(x, fmt):
    if fmt == 'cf32':
        return x
    f = x.astype(np.float32) * np.float32(scale_of(fmt))
    return (f[:, 0] + 1j * f[:, 1]).astype(np.complex64)


def copy_to_host(dst, dev_ptr):
    """hipMemcpy of the process's one HIP runtime (pycusdr_amd._lib loads it globally before the library)."""
    fn = C.CDLL(None).hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    assert fn(dst.ctypes.data, dev_ptr, dst.nbytes, 2) == 0  # hipMemcpyDeviceToHost


@pytest.mark.parametrize('fmt', ['cf32', 'sc16', 'sc8'])
@pytest.mark.parametrize('U,D', [(2, 3), (3, 5), (24, 25), (31, 64)])
def test_hold_plan_is_bit_exact(U, D, fmt):
    """h = ones(U), freq = 0: every branch is the one tap 1.0 and y[m] = x[(m D) div U] as bit patterns, signed zeros included;
    more than one workgroup, the last one partly live."""
    rs = np.random.RandomState(1)
    n = 1 << 13
    x = noise(rs, n, fmt)
    if fmt == 'cf32':
        x[5] = -0.0 + 0j
        x[6] = complex(-0.0, -0.0)
        x[7] = complex(0.0, -0.0)
    want_all = to_c64(x, fmt)
    nout = (n * U - 1) // D + 1
    q = np.arange(nout, dtype=np.int64) * D // U
    assert n - 1 - D < q[-1] <= n - 1
    # the identity on the CPU: 1.0 * x + (-0) is x, whatever the sign of a zero
    acc = np.float32(-0.0) + np.float32(1.0) * want_all.view(np.float32)
    assert np.array_equal(acc.view(np.uint32), want_all.view(np.uint32))
    cz = Channelizer(FS, D, np.ones(U, np.float32), [0.0], sample_format=fmt, sample_scale=scale_of(fmt), max_in=n, interp=U)
    tile, _ = cz.info()
    assert tile in (64 * U, 128 * U, 256 * U) and nout > tile
    y = cz.process(0, x, 0, nout)
    cz.close()
    assert y.shape == (1, nout)
    assert np.array_equal(bits(y[0]), bits(want_all[q])), (U, D, fmt)


@pytest.mark.parametrize('D,T,freqs,fmt', [(5, 23, [123.4e3, 0.0, -377.7e3], 'cf32'), (64, 1024, [1e5, 0.0], 'cf32'),
                                           (5, 23, [123.4e3, 0.0, -377.7e3], 'sc16')])
def test_forced_rational_kernel_at_interp_1_equals_the_integer_kernel(D, T, freqs, fmt):
    """The same plan through k_chzr (force_rational) and through k_chz: equal bits, for output counts around the rational
    kernel's tile.  Pins staging, indexing and summation order against the kernel that is already trusted."""
    rs = np.random.RandomState(2)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    kw = dict(sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 14)
    new = Channelizer(FS, D, h, freqs, interp=1, force_rational=True, **kw)
    old = Channelizer(FS, D, h, freqs, **kw)
    assert new.rational and not old.rational
    tile, _ = new.info()
    assert tile in (64, 128, 256)
    base = 1001
    for count in (tile - 1, tile, tile + 1, 2 * tile + 7):
        in_base, in_count = old.needed_input(base, count)
        assert (in_base, in_count) == new.needed_input(base, count)
        x = noise(rs, in_count, fmt)
        a = new.process(in_base, x, base, count)
        b = old.process(in_base, x, base, count)
        assert np.abs(b).max() > 0
        assert np.array_equal(bits(a), bits(b)), (D, T, count)
    new.close()
    old.close()


@pytest.mark.parametrize('U,D,T', [(3, 5, 23), (16, 25, 401)])
def test_pure_function_of_position(U, D, T):
    """One span from an out_base that is no multiple of U, computed whole, equals the same span in chunks around U and the tile,
    from odd and even in_base, from a window one sample wider than needed, in either output set, from host memory and from
    another channeliser's device_output pointer; and a channel's bits do not depend on the other channels of its plan."""
    rs = np.random.RandomState(3)
    h = (rs.uniform(-1, 1, T) * np.sqrt(U / T)).astype(np.float32)
    freqs = [123.4e3, 0.0, -377.7e3]
    cz = Channelizer(FS, D, h, freqs, max_in=1 << 15, interp=U)
    tile, cap = cz.info()
    assert tile in (64 * U, 128 * U, 256 * U) and cap == T
    base = 1001
    assert base % U
    counts = (1, U - 1, U, tile - 1, tile, tile + 1, 2 * tile + 7, 3)
    nout = sum(counts)
    in_base, in_count = cz.needed_input(base, nout)
    assert in_count <= 1 << 15
    # the input is itself a channeliser's output, left on the device: x on the host is a copy of it
    pre = Channelizer(FS, 2, [0.75], [0.0], max_in=2 * in_count)
    pre.process(0, noise(rs, 2 * in_count), 0, in_count, copy=False, buffer=0)
    dev_ptr, cnt = pre.device_output(0, 0)
    assert cnt == in_count
    x = np.empty(in_count, np.complex64)
    copy_to_host(x, dev_ptr)
    assert np.abs(x).min() > 0
    whole = cz.process(in_base, x, base, nout)
    parities, at = set(), base
    for i, n in enumerate(counts):
        b, c = cz.needed_input(at, n)
        if i % 3 == 2 and b > in_base:                       # a wider window than needed, from one sample earlier
            b, c = b - 1, c + 1
        parities.add(b & 1)
        part = cz.process(b, x[b - in_base:b - in_base + c], at, n, buffer=i & 1)
        assert np.array_equal(bits(part), bits(whole[:, at - base:at - base + n])), (i, n)
        cz.process(b, (dev_ptr + 8 * (b - in_base), c), at, n, copy=False, buffer=(i & 1) ^ 1)
        for k in range(3):
            ptr, cnt = cz.device_output((i & 1) ^ 1, k)
            assert cnt == n and ptr % 16 == 0
            got = np.empty(n, np.complex64)
            copy_to_host(got, ptr)
            assert np.array_equal(bits(got), bits(whole[k, at - base:at - base + n])), (i, n, k)
        at += n
    assert at == base + nout and parities == {0, 1}
    cz.close()
    pre.close()
    f16 = list(np.linspace(-450e3, 450e3, 13)) + freqs
    big = Channelizer(FS, D, h, f16, max_in=1 << 15, interp=U)
    y16 = big.process(in_base, x, base, nout)
    big.close()
    for k, f in enumerate(freqs):
        one = Channelizer(FS, D, h, [f], max_in=1 << 15, interp=U)
        y1 = one.process(in_base, x, base, nout)
        one.close()
        assert np.array_equal(bits(y1[0]), bits(whole[k])), k
        assert np.array_equal(bits(y1[0]), bits(y16[13 + k])), k


def stimulus(kind, rs, n, fmt, f0):
    i = np.arange(n)
    if kind == 'noise':
        x = 0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    else:                                                    # a full-scale tone inside the first channel
        x = 0.999 * np.exp(2j * np.pi * ((f0 + 3e3) / FS) * i) + 1e-3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    return quantise(x, fmt)


def freqs_for(K):
    if K == 3:
        return [151.7e3, 0.0, -288.8e3]
    return list(np.linspace(-0.47 * FS, 0.47 * FS, K - 2)) + [0.0, -FS / 2]


BOUND_CASES = [  # U, D, T, K, format
    (2, 3, 7, 3, 'cf32'), (3, 5, 3, 3, 'sc16'), (16, 25, 401, 3, 'cf32'), (31, 64, 1024, 16, 'cf32'), (32, 63, 1000, 5, 'sc8'),
]


@pytest.mark.parametrize('kind', ['noise', 'tone'])
@pytest.mark.parametrize('case', range(len(BOUND_CASES)))
def test_device_within_the_derived_bound_of_the_model(case, kind):
    U, D, T, K, fmt = BOUND_CASES[case]
    Tb = -(-T // U)
    rs = np.random.RandomState(200 + case)
    h = design_taps(D, 16, interp=U) if T == D * 16 + 1 else (rs.uniform(-1, 1, T) * np.sqrt(U / T)).astype(np.float32)
    assert len(h) == T
    freqs = freqs_for(K)
    cz = Channelizer(FS, D, h, freqs, sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 16, interp=U)
    tile, _ = cz.info()
    nout = 3 * tile + 5
    out_base = 1001 if case % 2 == 0 else (1 << 40) // D + 3
    in_base, in_count = cz.needed_input(out_base, nout)
    assert in_count <= 1 << 16
    x = stimulus(kind, rs, in_count, fmt, freqs[0])
    y = cz.process(in_base, x, out_base, nout)
    ref, S = cz.model(in_base, x, out_base, nout)
    cz.close()
    assert np.all(S > 0) and np.abs(ref).max() > 0
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    c = float((err / (EPS * S)).max())
    print(f'case {case} {kind}: (U, D, T) = ({U}, {D}, {T}) Tb {Tb} K {K} {fmt} tile {tile} out_base {out_base}: '
          f'worst c = {c:.2f} (ceiling {3 * Tb + 24})')
    assert c <= 3 * Tb + 24
    assert c <= C_BOUND


def test_positions_below_zero_read_zeros():
    """The stream x at out_base 0 equals the stream [Z zeros, x] at the out_base Z maps to (Z U divisible by D; freq = 0: no phase
    moves with the shift); both channels are within the bound of the model; output 0 is exactly h[0] x[0]."""
    rs = np.random.RandomState(4)
    U, D, T = 3, 5, 23
    Z = D
    assert Z * U % D == 0
    h = rs.uniform(-1, 1, T).astype(np.float32)
    x = noise(rs, 2000)
    cz = Channelizer(FS, D, h, [0.0, 1.0e5], max_in=4096, interp=U)
    nout = 900                                               # more than one tile
    assert nout > cz.info()[0]
    a = cz.process(0, x, 0, nout)
    b = cz.process(0, np.r_[np.zeros(Z, np.complex64), x], Z * U // D, nout)
    ref, S = cz.model(0, x, 0, nout)
    cz.close()
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert a[0, 0] == np.complex64(complex(h[0] * x[0].real, h[0] * x[0].imag))
    err = np.maximum(np.abs(a.real - ref.real), np.abs(a.imag - ref.imag))
    assert np.all(err <= (3 * -(-T // U) + 24) * EPS * S)


def test_every_misuse_is_an_error_code():
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    U, D, T = 3, 5, 10                                       # Tb = 4
    taps = np.linspace(0.1, 0.9, 64).astype(np.float32)
    words = np.array([1 << 60, 0], dtype=np.uint64)
    pre = Channelizer(FS, 2, [1.0], [0.0], max_in=8192)      # 4096 complex64 in device memory: a channeliser's output set
    pre.process(0, np.zeros(8191, np.complex64), 0, 4096, copy=False, buffer=0)
    dev_ptr = pre.device_output(0, 0)[0]
    out = np.empty((2, 1024), np.complex64)
    h = C.c_void_p()
    assert lib.mfb_channelizer_create(C.byref(h), 0, 4, 64, 4096, 1024) == OK

    def params(**kw):
        d = dict(in_base=0, out_base=0, device_input=dev_ptr, in_count=4096, out_count=1000, input=2, buffer=0)
        d.update(kw)
        return _lib.ChannelizerParams(**d)

    def plan(hh, u=U, d=D, nt=T, nc=2, fmt=0, scale=1.0, t=taps, w=words):
        return lib.mfb_channelizer_set_plan_rational(hh, u, d, t.ctypes.data if t is not None else None, nt,
                                                     w.ctypes.data if w is not None else None, nc, fmt, scale)

    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE          # _begin without a plan
    assert plan(None) == ARG and plan(h, t=None) == ARG and plan(h, w=None) == ARG
    for u, d in ((2, 4), (15, 25), (6, 9)):                                  # a common factor
        assert plan(h, u=u, d=d, nt=40) == ARG, (u, d)
    for u, d in ((5, 5), (7, 5), (32, 31), (2, 2)):                          # U >= D
        assert plan(h, u=u, d=d, nt=40) == ARG, (u, d)
    assert plan(h, u=3, d=5, nt=2) == ARG                                    # T < U
    assert plan(h, fmt=3) == ARG and plan(h, fmt=1, scale=0.3) == ARG
    assert plan(h, nt=65) == ARG and plan(h, nc=5) == ARG                    # more than the handle was created for
    for u, d in ((33, 64), (0, 5), (-1, 5), (3, 65), (1, 1)):                # beyond the limits
        assert plan(h, u=u, d=d, nt=40) == UNSUP, (u, d)
    assert plan(h, nt=1025) == UNSUP and plan(h, nc=17) == UNSUP
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE          # every refusal left the handle without a plan
    assert plan(h) == OK
    a, b = C.c_int(), C.c_int()
    assert lib.mfb_channelizer_info(h, C.byref(a), C.byref(b)) == OK and a.value == U * 256 and b.value == 64
    # the window rule, one sample short at either end: outputs 100 .. 299 read inputs 100 * 5 div 3 - 3 = 163 .. 299 * 5 div 3 = 498
    need = dict(out_base=100, out_count=200)
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=163, in_count=336, **need))) == OK
    assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=164, in_count=335, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=163, in_count=335, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=1, in_count=4000, out_base=0, out_count=10))) == ARG     # position 0 is not below 0
    for kw in (dict(in_count=0), dict(out_count=0), dict(in_base=-1), dict(out_base=-1), dict(buffer=2), dict(input=3),
               dict(device_input=None), dict(device_input=dev_ptr + 4), dict(in_count=4097), dict(out_count=1025)):
        assert lib.mfb_channelizer_begin(h, C.byref(params(**kw))) == ARG, kw
    for kw in (dict(in_count=(1 << 24) + 1), dict(out_count=(1 << 22) + 1), dict(in_base=1 << 62),
               dict(out_base=(1 << 62) // D + 1)):
        assert lib.mfb_channelizer_begin(h, C.byref(params(**kw))) == UNSUP, kw
    # in flight
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
    assert plan(h) == STATE
    assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK
    # an integer plan takes the handle back, and its own window rule with it: outputs 100 .. 299 read 100 * 5 - 9 .. 299 * 5
    assert lib.mfb_channelizer_set_plan(h, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == OK
    assert lib.mfb_channelizer_info(h, C.byref(a), None) == OK and a.value == 256
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=163, in_count=336, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=491, in_count=1005, **need))) == OK
    assert lib.mfb_channelizer_end(h, None) == OK
    assert lib.mfb_channelizer_destroy(h) == OK
    pre.close()


def test_two_stages_on_device_pointers():
    """1 MHz -> 153.6 kHz, 96/625 as factor_rate splits it: two carriers through the first stage, each then through a second
    stage (one channel, freq 0) that reads the first stage's device_output pointer.  Against the same two stages of the float64
    model: the second stage's own bound, plus its sum |h| times the first stage's bound."""
    rs = np.random.RandomState(6)
    (U1, D1), (U2, D2) = stages = factor_rate(1e6, 153600)
    assert stages == [(4, 25), (24, 25)]
    h1, h2 = design_taps(D1, interp=U1), design_taps(D2, interp=U2)
    s1 = Channelizer(1e6, D1, h1, [200e3, -310e3], max_in=1 << 13, interp=U1)
    s2 = Channelizer(1e6 * U1 / D1, D2, h2, [0.0], max_in=1 << 10, interp=U2)
    base2, n2 = 517, 300
    base1, n1 = s2.needed_input(base2, n2)
    base0, n0 = s1.needed_input(base1, n1)
    i = np.arange(base0, base0 + n0)
    x = (0.4 * np.exp(2j * np.pi * 0.2003 * i) + 0.4 * np.exp(-2j * np.pi * 0.3102 * i)
         + 0.05 * (rs.standard_normal(n0) + 1j * rs.standard_normal(n0))).astype(np.complex64)
    s1.process(base0, x, base1, n1, copy=False, buffer=1)
    ref1, S1 = s1.model(base0, x, base1, n1)
    bound1 = (3 * s1.Tb + 24) * EPS * S1
    for k in range(2):
        ptr, cnt = s1.device_output(1, k)
        assert cnt == n1
        y = s2.process(base1, (ptr, n1), base2, n2)
        ref2, S2 = s2._model_rational(base1, ref1[k], base2, n2)      # (model() would round the first stage to complex64)
        err = np.maximum(np.abs(y.real - ref2.real), np.abs(y.imag - ref2.imag))
        bound = (3 * s2.Tb + 24) * EPS * S2 + np.abs(h2).astype(np.float64).sum() * bound1.max()
        print(f'carrier {k}: worst error {err.max():.3e}, its bound {bound[err.argmax()]:.3e}, largest output {np.abs(ref2).max():.3f}')
        assert np.abs(ref2).max() > 0.3                      # the carrier came through both pass bands
        assert np.all(err <= bound)
    s1.close()
    s2.close()
