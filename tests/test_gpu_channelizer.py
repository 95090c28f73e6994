"""The device channeliser (csrc/channelize_kernels.hpp, mfb_channelizer_*) against its contract: exact where nothing rounds, a
pure function of the absolute position bit for bit, within a derived bound of the float64 model (``Channelizer(backend='host')``),
an error code for every misuse, and device memory returned.

The error bound.  Per component |device - model| <= c * 2^-24 * S_m with S_m = sum_t |h[t]| |x[m D - t]|.  First-order worst case of
the form the kernel computes (modulated taps, one rotation per output): a sequential fp32 sum of 2 T products per component over
terms bounded by sqrt(2) S gives 2.83 T; the tap phasor and the rotation phasor, each within 4 * 2^-24 per component
(mod_kernels.hpp), the tap's rounding and the rotation's products and sum add less than 24: c <= 3 T + 24.  Every case asserts that
ceiling for its own T.  C_BOUND pins twice the worst c measured over all cases (profiles/channelizer.md has the figure per T)."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd.channelizer import FORMATS, Channelizer, design_taps

pytestmark = pytest.mark.gpu

FS = 1.0e6
EPS = 2.0 ** -24
T_MAX = 1024
C_BOUND = 7                       # twice the worst measured c (3.10, case 2: T = 5, D = 8, K = 16, a tone), rounded up
assert C_BOUND <= 3 * T_MAX + 24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def noise(rs, n, fmt):
    x = 0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    return quantise(x, fmt)


def quantise(x, fmt):
    """The stimulus in the plan's sample format: complex64, or integers below full scale."""
    if fmt == 'cf32':
        return x.astype(np.complex64)
    full = 32767 if fmt == 'sc16' else 127
    q = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) * full), -full - 1, full)
    return q.astype(np.int16 if fmt == 'sc16' else np.int8)


def scale_of(fmt):
    return {'cf32': 1.0, 'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}[fmt]


@pytest.mark.parametrize('fmt', ['cf32', 'sc16', 'sc8'])
def test_identity_plan_is_bit_exact(fmt):
    """h = [1], freq = 0: y[m] = x[m D] as bit patterns; the integer formats against raw.astype(float32) * scale."""
    rs = np.random.RandomState(1)
    n = 1 << 12
    x = noise(rs, n, fmt)
    if fmt == 'cf32':
        want_all = x
        x[5] = -0.0 + 0j                                     # a signed zero keeps its sign
        x[6] = complex(-0.0, -0.0)
    else:
        f = x.astype(np.float32) * np.float32(scale_of(fmt))
        want_all = (f[:, 0] + 1j * f[:, 1]).astype(np.complex64)
    for D in (2, 5, 64):
        cz = Channelizer(FS, D, [1.0], [0.0], sample_format=fmt, sample_scale=scale_of(fmt), max_in=n)
        nout = (n - 1) // D + 1
        y = cz.process(0, x, 0, nout)
        cz.close()
        assert y.shape == (1, nout)
        assert np.array_equal(bits(y[0]), bits(want_all[::D])), (fmt, D)


def test_positions_below_zero_read_zeros():
    """The stream x at out_base 0 equals the stream [Z zeros, x] at out_base Z / D (freq = 0: no phase moves with the shift), and
    the very first output is the one product h[0] x[0]."""
    rs = np.random.RandomState(2)
    D, T, Z = 4, 23, 64
    h = rs.uniform(-1, 1, T).astype(np.float32)
    x = noise(rs, 1000, 'cf32')
    cz = Channelizer(FS, D, h, [0.0, 1.0e5], max_in=2048)
    nout = 200
    a = cz.process(0, x, 0, nout)
    b = cz.process(0, np.r_[np.zeros(Z, np.complex64), x], Z // D, nout)
    ref, S = cz.model(0, x, 0, nout)
    cz.close()
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert a[0, 0] == np.complex64(complex(h[0] * x[0].real, h[0] * x[0].imag))
    assert np.abs(a - ref).max() <= (3 * T + 24) * EPS * S.max()


def test_pure_function_of_position():
    """One span computed whole equals the same span in uneven chunks, from odd and even in_base, for out_count around the tile, in
    either output set and from device memory, bit for bit."""
    import torch
    rs = np.random.RandomState(3)
    D, T = 5, 23
    h = rs.uniform(-1, 1, T).astype(np.float32)
    freqs = [123.4e3, 0.0, -377.7e3]
    cz = Channelizer(FS, D, h, freqs, max_in=1 << 14)
    tile, cap = cz.info()
    assert tile in (64, 128, 256) and cap == T
    base = 1001
    total = 0
    counts = (1, tile - 1, tile, tile + 1, 2 * tile + 7, 3, 40)
    nout = sum(counts)
    in_base, in_count = cz.needed_input(base, nout)
    x = noise(rs, in_count, 'cf32')
    whole = cz.process(in_base, x, base, nout)
    dev = torch.from_numpy(x).cuda()
    parities = set()
    at = base
    for i, n in enumerate(counts):
        b, c = cz.needed_input(at, n)
        if i % 3 == 2 and b > in_base:                       # a wider window than needed, from one sample earlier
            b, c = b - 1, c + 1
        parities.add(b & 1)
        part = cz.process(b, x[b - in_base:b - in_base + c], at, n, buffer=i & 1)
        assert np.array_equal(bits(part), bits(whole[:, at - base:at - base + n])), (i, n)
        # the same chunk from device memory, left on the device and fetched from the output set
        cz.process(b, (dev.data_ptr() + 8 * (b - in_base), c), at, n, copy=False, buffer=(i & 1) ^ 1)
        for k in range(3):
            ptr, cnt = cz.device_output((i & 1) ^ 1, k)
            assert cnt == n and ptr % 16 == 0
            got = np.empty(n, np.complex64)
            _copy_to_host(got, ptr)
            assert np.array_equal(bits(got), bits(whole[k, at - base:at - base + n])), (i, n, k)
        at += n
        total += n
    assert total == nout and parities == {0, 1}
    cz.close()
    # channel k of a K = 1 plan against the same word inside a K = 3 and a K = 16 plan
    f16 = list(np.linspace(-450e3, 450e3, 13)) + freqs
    big = Channelizer(FS, D, h, f16, max_in=1 << 14)
    y16 = big.process(in_base, x, base, nout)
    big.close()
    for k, f in enumerate(freqs):
        one = Channelizer(FS, D, h, [f], max_in=1 << 14)
        y1 = one.process(in_base, x, base, nout)
        one.close()
        assert np.array_equal(bits(y1[0]), bits(whole[k])), k
        assert np.array_equal(bits(y1[0]), bits(y16[13 + k])), k


def _copy_to_host(dst, dev_ptr):
    """hipMemcpy of the process's one HIP runtime (pycusdr_amd._lib loads it globally before the library)."""
    fn = C.CDLL(None).hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    assert fn(dst.ctypes.data, dev_ptr, dst.nbytes, 2) == 0  # hipMemcpyDeviceToHost


def words_for(K, i):
    """Positive and negative tuning, 0, and words next to 2^63 (fs / 2)."""
    if K == 1:
        return [[217.3e3], [-401.9e3], [0.4999999 * FS], [-FS / 2]][i % 4]
    if K == 3:
        return [151.7e3, -288.8e3, 0.49999993 * FS]
    return list(np.linspace(-0.47 * FS, 0.47 * FS, 12)) + [0.0, -FS / 2, 0.4999999 * FS, -0.4999998 * FS]


def stimulus(kind, rs, n, fmt, freqs):
    i = np.arange(n)
    if kind == 'noise':
        x = 0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    elif kind == 'tone':                                     # full scale, in the neighbouring channel
        x = 0.999 * np.exp(2j * np.pi * ((freqs[0] + 60e3) / FS) * i) + 1e-3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))
    else:                                                    # zero except one burst
        x = np.zeros(n, dtype=np.complex128)
        x[n // 3:n // 3 + 37] = 0.7 * (rs.standard_normal(37) + 1j * rs.standard_normal(37))
    return quantise(x, fmt)


CASES = [  # T (None: 4 D + 3), D, K, format, stimulus, large base
    (1, 2, 1, 'cf32', 'noise', False), (2, 3, 3, 'sc16', 'noise', True), (5, 8, 16, 'cf32', 'tone', False),
    (17, 16, 3, 'sc8', 'burst', True), (None, 2, 16, 'cf32', 'noise', True), (None, 3, 1, 'cf32', 'tone', False),
    (None, 8, 3, 'sc16', 'burst', False), (None, 16, 16, 'cf32', 'noise', True), (None, 64, 3, 'cf32', 'tone', True),
    (1024, 64, 16, 'cf32', 'noise', False), (1024, 2, 1, 'sc16', 'noise', True), (1024, 16, 3, 'cf32', 'burst', False),
    (17, 64, 1, 'sc8', 'noise', False), (5, 16, 16, 'sc16', 'tone', True), (2, 8, 1, 'cf32', 'noise', True),
    (1, 3, 3, 'sc8', 'tone', False),
]
WORST = {}


@pytest.mark.parametrize('case', range(len(CASES)))
def test_device_within_the_derived_bound_of_the_model(case):
    T, D, K, fmt, kind, large = CASES[case]
    T = 4 * D + 3 if T is None else T
    rs = np.random.RandomState(100 + case)
    h = design_taps(D, 1)[:T] if T <= D + 1 else rs.uniform(-1, 1, T).astype(np.float32) / np.sqrt(T)
    freqs = words_for(K, case)
    nout = 300                                               # more than one tile of 256
    out_base = ((1 << 40) // D + 3) if large else 0
    cz = Channelizer(FS, D, h, freqs, sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 16)
    in_base, in_count = cz.needed_input(out_base, nout)
    assert in_count <= 1 << 16
    x = stimulus(kind, rs, in_count, fmt, freqs)
    y = cz.process(in_base, x, out_base, nout)
    ref, S = cz.model(in_base, x, out_base, nout)
    cz.close()
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    dead = S == 0
    assert np.all(y[:, dead] == 0)                           # nothing read, nothing computed
    c = float((err[:, ~dead] / (EPS * S[~dead])).max())
    WORST[T] = max(WORST.get(T, 0.0), c)
    print(f'case {case}: T {T} D {D} K {K} {fmt} {kind} out_base {out_base}: worst c = {c:.2f} (ceiling {3 * T + 24}); '
          f'worst per T so far {dict(sorted(WORST.items()))}')
    assert np.abs(ref).max() > 0
    assert c <= 3 * T + 24
    assert c <= C_BOUND


def _handle(lib, max_channels=4, max_taps=64, max_in=4096, max_out=1024):
    h = C.c_void_p()
    assert lib.mfb_channelizer_create(C.byref(h), 0, max_channels, max_taps, max_in, max_out) == _lib.MFB_OK
    return h


def test_every_misuse_is_an_error_code():
    import torch
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    D, T = 4, 9
    taps = np.linspace(0.1, 0.9, T).astype(np.float32)
    words = np.array([1 << 60, 0], dtype=np.uint64)
    dev = torch.zeros(4096, dtype=torch.complex64, device='cuda')
    out = np.empty((2, 1024), np.complex64)
    hp = C.c_void_p()

    def params(**kw):
        d = dict(in_base=0, out_base=0, device_input=dev.data_ptr(), in_count=4096, out_count=1000, input=2, buffer=0)
        d.update(kw)
        return _lib.ChannelizerParams(**d)

    def plan(h, decim=D, t=taps, nt=T, w=words, nc=2, fmt=0, scale=1.0):
        return lib.mfb_channelizer_set_plan(h, decim, t.ctypes.data if t is not None else None, nt, w.ctypes.data if w is not None else None,
                                            nc, fmt, scale)

    def good(h):
        """The handle still works."""
        assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
        assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK

    # create
    assert lib.mfb_channelizer_create(None, 0, 1, 1, 1, 1) == ARG
    for a in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.mfb_channelizer_create(C.byref(hp), 0, *a) == ARG and not hp.value
    for a in ((17, 1, 1, 1), (1, 1025, 1, 1), (1, 1, (1 << 24) + 1, 1), (1, 1, 1, (1 << 22) + 1)):
        assert lib.mfb_channelizer_create(C.byref(hp), 0, *a) == UNSUP and not hp.value
    assert lib.mfb_channelizer_create(C.byref(hp), 1 << 20, 1, 1, 1, 1) == ARG
    assert lib.mfb_channelizer_destroy(None) == ARG

    h = _handle(lib)
    # before a plan
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE
    assert lib.mfb_channelizer_info(h, None, None) == STATE
    assert lib.mfb_channelizer_end(h, None) == STATE
    # set_plan
    assert plan(None) == ARG and plan(h, t=None) == ARG and plan(h, w=None) == ARG
    assert plan(h, nt=0) == ARG and plan(h, nc=0) == ARG
    assert plan(h, fmt=3) == ARG
    assert plan(h, fmt=1, scale=0.3) == ARG and plan(h, fmt=2, scale=-0.5) == ARG and plan(h, fmt=1, scale=float('inf')) == ARG
    for bad in (np.nan, np.inf):
        t2 = taps.copy()
        t2[3] = bad
        assert plan(h, t=t2) == ARG
    assert plan(h, t=np.ones(65, np.float32), nt=65) == ARG                  # more than the handle was created for
    assert plan(h, w=np.zeros(5, np.uint64), nc=5) == ARG
    for decim in (1, 0, 65):
        assert plan(h, decim=decim) == UNSUP
    assert plan(h, t=np.ones(1025, np.float32), nt=1025) == UNSUP
    assert plan(h, w=np.zeros(17, np.uint64), nc=17) == UNSUP
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE          # every refusal left the handle without a plan
    assert plan(h) == OK
    good(h)
    # begin: ARG
    assert lib.mfb_channelizer_begin(None, C.byref(params())) == ARG
    assert lib.mfb_channelizer_begin(h, None) == ARG
    for kw in (dict(in_count=0), dict(out_count=0), dict(in_base=-1), dict(out_base=-1), dict(buffer=2), dict(buffer=-1), dict(input=3),
               dict(device_input=None), dict(device_input=dev.data_ptr() + 4), dict(in_count=4097), dict(out_count=1025)):
        assert lib.mfb_channelizer_begin(h, C.byref(params(**kw))) == ARG, kw
    # the uncovered-input rule, one sample short at either end: outputs 100 .. 299 read inputs 392 .. 1196
    need = dict(out_base=100, out_count=200)
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=392, in_count=805, **need))) == OK
    assert lib.mfb_channelizer_end(h, None) == OK
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=393, in_count=804, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=392, in_count=804, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=1, in_count=4000, out_base=0, out_count=10))) == ARG     # position 0 is not below 0
    # begin: UNSUPPORTED
    for kw in (dict(in_count=(1 << 24) + 1), dict(out_count=(1 << 22) + 1), dict(in_base=1 << 62), dict(out_base=(1 << 62) // D)):
        assert lib.mfb_channelizer_begin(h, C.byref(params(**kw))) == UNSUP, kw
    # a pinned input that was never asked for; then asked for
    assert lib.mfb_channelizer_begin(h, C.byref(params(input=1))) == STATE
    nbytes = C.c_size_t()
    assert lib.mfb_channelizer_input_buffer(h, 1, None, C.byref(nbytes)) == ARG
    assert lib.mfb_channelizer_input_buffer(h, 2, C.byref(hp), C.byref(nbytes)) == ARG
    assert lib.mfb_channelizer_input_buffer(h, 1, C.byref(hp), C.byref(nbytes)) == OK and nbytes.value == 4096 * 8
    good(h)
    # STATE
    ptr, cnt = C.c_void_p(), C.c_int64()
    assert lib.mfb_channelizer_device_output(h, 1, 0, C.byref(ptr), C.byref(cnt)) == STATE      # set 1 was never written
    assert lib.mfb_channelizer_device_output(h, 0, 2, C.byref(ptr), C.byref(cnt)) == STATE      # the plan has two channels
    assert lib.mfb_channelizer_device_output(h, 0, -1, C.byref(ptr), C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 2, 0, C.byref(ptr), C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 0, 0, None, C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 0, 1, C.byref(ptr), C.byref(cnt)) == OK and cnt.value == 1000 and ptr.value % 16 == 0
    assert lib.mfb_channelizer_end(h, None) == STATE
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
    assert lib.mfb_channelizer_begin(h, C.byref(params(buffer=1))) == STATE
    assert plan(h) == STATE
    assert lib.mfb_channelizer_device_output(h, 0, 0, C.byref(ptr), C.byref(cnt)) == STATE      # in flight
    assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK
    good(h)
    assert lib.mfb_channelizer_destroy(h) == OK


def test_cycles_return_device_memory():
    import torch
    rs = np.random.RandomState(9)
    n = 1 << 20
    x = noise(rs, n, 'sc16')
    taps = design_taps(4)

    def cycle():
        cz = Channelizer(FS, 4, taps, [1e5, -2e5, 0.0, 3e5], sample_format='sc16', sample_scale=2.0 ** -15, max_in=n, max_out=n // 4)
        cz.process(0, x, 0, n // 4 - 16)
        cz.close()
    assert 20 * 2 * 4 * (n // 4) * 8 > (32 << 20)             # the output sets alone would cross the bound
    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f'20 cycles: device free {free0 >> 20} -> {free1 >> 20} MiB')
    assert abs(free0 - free1) < (32 << 20), (free0, free1)


def test_formats_table_matches_the_header():
    assert FORMATS == {'cf32': 0, 'sc16': 1, 'sc8': 2}
