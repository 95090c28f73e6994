"""The uniform polyphase channeliser on the device (csrc/channelize_uniform_kernels.hpp, mfb_channelizer_create_uniform /
_set_plan_uniform) against its contract: within a derived bound of the float64 model (``UniformChannelizer.model``, the arithmetic
of ``Channelizer.model`` on the exact raster words), a pure function of the absolute position bit for bit whatever the cut, the
window and the selection, equal to the direct kernel within both pinned constants, an error code for every misuse, and device
memory returned.

The error bound.  Per component |device - model| <= c * 2^-24 * S_m with S_m = sum_t |h[t]| |x[m D - t]|.  First order, for the
kernel as built: a branch sum is a chain of at most ceil(T / M) fused multiply-adds per component, error at most ceil(T / M) u times
the branch's own sum of |h| |x| (the two components' sums combine by the triangle inequality), so ceil(T / M) u S over all
branches.  Inside the transform every value is at most S in modulus; a level of additions rounds by u relative, the
(1 +- i) / sqrt(2) products of the radix-8 butterfly by 3 u (an addition, a product, the constant), a twiddle product with fused
multiply-adds by 2 u and its table entry by u.  A radix-4 pass, 2 bits of M: 2 + 3 = 5 u; a radix-8 pass, 3 bits: 3 + 3 + 3 = 9 u; at
most 3 u per bit, passed on with gain 1.  Second-order terms: 2.  So c <= ceil(T / M) + 3 log2 M + 2, asserted by every case for its
own (M, T).  C_BOUND pins twice the worst c measured over all cases (profiles/channelizer_uniform.md has the figure per (M, T))."""
import ctypes as C

import numpy as np
import pytest

from pycusdr_amd import _lib
from pycusdr_amd.channelizer import Channelizer, UniformChannelizer, design_taps

pytestmark = pytest.mark.gpu

FS = 1.024e6                      # b fs / M quantises to the exact word for every bin of M = 8 and 16 (test_channelizer_uniform_host.py)
EPS = 2.0 ** -24
C_BOUND = 4                       # twice the worst measured c (1.97, M = 256, D = 2, T = 300 from out_base 0), rounded up
DIRECT_C_BOUND = 7                # the direct kernel's pinned constant (tests/test_gpu_channelizer.py)


def ceiling(M, T):
    return -(-T // M) + 3 * int(np.log2(M)) + 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def quantise(x, fmt):
    """The stimulus in the plan's sample format: complex64, or integers below full scale."""
    if fmt == 'cf32':
        return x.astype(np.complex64)
    full = 32767 if fmt == 'sc16' else 127
    q = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) * full), -full - 1, full)
    return q.astype(np.int16 if fmt == 'sc16' else np.int8)


def noise(rs, n, fmt='cf32'):
    return quantise(0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n)), fmt)


def scale_of(fmt):
    return {'cf32': 1.0, 'sc16': 2.0 ** -15, 'sc8': 2.0 ** -7}[fmt]


def spread(M):
    """All bins, or 16 spread ones where M > 16: both ends, the middle, a neighbour of 0, and twelve more, in no order."""
    if M <= 16:
        return list(range(M))
    b = [0, M - 1, M // 2, 1]
    b += [int(k) for k in np.random.RandomState(M).permutation(M) if k not in b][:12]
    return b


def _copy_to_host(dst, dev_ptr):
    """hipMemcpy of the process's one HIP runtime (pycusdr_amd._lib loads it globally before the library)."""
    fn = C.CDLL(None).hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    assert fn(dst.ctypes.data, dev_ptr, dst.nbytes, 2) == 0  # hipMemcpyDeviceToHost


SHAPES = [(8, 8, 1), (8, 2, 8), (8, 3, 37), (16, 16, 129), (16, 5, 17), (32, 32, 32), (32, 7, 33), (64, 32, 513), (64, 48, 1025),
          (64, 64, 4096), (128, 96, 2049), (256, 256, 4096), (256, 128, 257), (256, 2, 300)]
CASES = [(s, large, 'cf32') for s in SHAPES for large in (False, True)]
CASES += [((8, 3, 37), True, 'sc16'), ((8, 3, 37), False, 'sc8'), ((64, 32, 513), False, 'sc16'), ((64, 32, 513), True, 'sc8'),
          ((256, 2, 300), True, 'sc16'), ((256, 2, 300), False, 'sc8')]
WORST = {}


@pytest.mark.parametrize('case', range(len(CASES)))
def test_device_within_the_derived_bound_of_the_model(case):
    (M, D, T), large, fmt = CASES[case]
    rs = np.random.RandomState(500 + case)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    sel = spread(M)
    out_base = ((1 << 40) // D + 3) if large else 0
    uz = UniformChannelizer(FS, M, D, h, bins=sel, sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 17)
    F, cap = uz.info()
    assert cap == T and (F % 16 == 0 or F in (4, 8)) and F * M % 256 == 0
    nout = 2 * F + 5
    in_base, in_count = uz.needed_input(out_base, nout)
    assert in_count <= 1 << 17
    x = noise(rs, in_count, fmt)
    y = uz.process(in_base, x, out_base, nout)
    ref, S = uz.model(in_base, x, out_base, nout)
    uz.close()
    assert y.shape == ref.shape == (len(sel), nout) and S.min() > 0           # no output is left out of the comparison
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    c = float((err / (EPS * S)).max())
    WORST[(M, T)] = max(WORST.get((M, T), 0.0), c)
    print(f'case {case}: M {M} D {D} T {T} F {F} {fmt} out_base {out_base}: worst c = {c:.2f} (ceiling {ceiling(M, T)}); '
          f'worst per (M, T) so far {dict(sorted(WORST.items()))}')
    assert c <= ceiling(M, T)
    assert c <= C_BOUND


@pytest.mark.parametrize('M, D, T', [(32, 7, 33), (64, 64, 200)])
def test_pure_function_of_position(M, D, T):
    """One span computed whole equals the same span in uneven chunks around F, from odd and even in_base, from a longer input
    window, in either output set, from device memory, and with all bins, one bin or a permuted subset selected: bit for bit."""
    import torch
    rs = np.random.RandomState(M)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    every = UniformChannelizer(FS, M, D, h, max_in=1 << 17)
    F, _ = every.info()
    base = 1001
    counts = (1, F - 1, F, F + 1, 2 * F + 7, 3, 40)
    nout = sum(counts)
    in_base, in_count = every.needed_input(base, nout)
    x = noise(rs, in_count)
    whole = every.process(in_base, x, base, nout)
    assert whole.shape == (M, nout)
    dev = torch.from_numpy(x).cuda()
    subset = [M - 3, 5, M // 2, 0, 11, M - 1, 6]
    one = UniformChannelizer(FS, M, D, h, bins=[M - 3], max_in=1 << 17)
    some = UniformChannelizer(FS, M, D, h, bins=subset, max_in=1 << 17)
    assert one.info() == some.info() == every.info()
    assert np.array_equal(bits(one.process(in_base, x, base, nout)), bits(whole[[M - 3]]))
    assert np.array_equal(bits(some.process(in_base, x, base, nout)), bits(whole[subset]))
    parities, wider, at = set(), 0, base
    for i, n in enumerate(counts):
        b, c = every.needed_input(at, n)
        if i % 3 == 2 and b > in_base:                       # a wider window than needed: one sample earlier, two later
            b, c = b - 1, min(c + 3, in_base + in_count - b + 1)
            wider += 1
        parities.add(b & 1)
        want = whole[:, at - base:at - base + n]
        part = every.process(b, x[b - in_base:b - in_base + c], at, n, buffer=i & 1)
        assert np.array_equal(bits(part), bits(want)), (i, n)
        assert np.array_equal(bits(some.process(b, x[b - in_base:b - in_base + c], at, n, buffer=(i & 1) ^ 1)), bits(want[subset])), (i, n)
        assert np.array_equal(bits(one.process(b, x[b - in_base:b - in_base + c], at, n)), bits(want[[M - 3]])), (i, n)
        # the same chunk from device memory, left on the device and fetched from the output set
        every.process(b, (dev.data_ptr() + 8 * (b - in_base), c), at, n, copy=False, buffer=(i & 1) ^ 1)
        for k in (0, 1, M // 2, M - 1):
            ptr, cnt = every.device_output((i & 1) ^ 1, k)
            assert cnt == n and ptr % 16 == 0
            got = np.empty(n, np.complex64)
            _copy_to_host(got, ptr)
            assert np.array_equal(bits(got), bits(want[k])), (i, n, k)
        at += n
    assert at == base + nout and parities == {0, 1} and wider >= 2
    for z in (every, one, some):
        z.close()


@pytest.mark.parametrize('M, D, T, Z', [(8, 4, 23, 64), (16, 5, 17, 80)])
def test_positions_below_zero_read_zeros(M, D, T, Z):
    """The stream x at out_base 0 equals the stream [Z zeros, x] at out_base Z / D, Z a multiple of lcm(D, M): the shift moves no
    bin's phase, so every bin may be compared."""
    rs = np.random.RandomState(2)
    assert Z % D == 0 and Z % M == 0
    h = rs.uniform(-1, 1, T).astype(np.float32)
    x = noise(rs, 1500)
    uz = UniformChannelizer(FS, M, D, h, max_in=2048)
    nout = 270
    a = uz.process(0, x, 0, nout)
    b = uz.process(0, np.r_[np.zeros(Z, np.complex64), x], Z // D, nout)
    ref, S = uz.model(0, x, 0, nout)
    uz.close()
    assert np.array_equal(bits(a), bits(b))
    assert np.all(np.maximum(np.abs(a.real - ref.real), np.abs(a.imag - ref.imag)) <= ceiling(M, T) * EPS * S)
    # frame 0 holds one value and zeros, which every addition passes on exactly: bin 0's first output is that product
    assert a[0, 0] == np.complex64(complex(h[0] * x[0].real, h[0] * x[0].imag))


@pytest.mark.parametrize('fmt', ['sc16', 'sc8'])
def test_integer_formats_equal_their_floats(fmt):
    """An sc16 / sc8 plan gives, bit for bit, what a cf32 plan gives on raw.astype(float32) * scale."""
    rs = np.random.RandomState(7)
    M, D, T = 32, 7, 33
    h = rs.uniform(-1, 1, T).astype(np.float32)
    for scale in (scale_of(fmt), 2.0 ** -3):
        a = UniformChannelizer(FS, M, D, h, sample_format=fmt, sample_scale=scale, max_in=1 << 13)
        b = UniformChannelizer(FS, M, D, h, max_in=1 << 13)
        F, _ = a.info()
        nout = 2 * F + 5
        in_base, n = a.needed_input(77, nout)
        raw = noise(rs, n, fmt)
        f = raw.astype(np.float32) * np.float32(scale)
        ya = a.process(in_base, raw, 77, nout)
        yb = b.process(in_base, (f[:, 0] + 1j * f[:, 1]).astype(np.complex64), 77, nout)
        assert a.input_buffer(0).dtype == raw.dtype
        a.close()
        b.close()
        assert np.array_equal(bits(ya), bits(yb)), scale


@pytest.mark.parametrize('M, D, T', [(8, 3, 37), (16, 5, 17)])
def test_two_device_implementations_agree(M, D, T):
    """The uniform kernel and the direct kernel on the same words (``Channelizer(freqs_hz=b fs / M)``, exact at this fs) are each
    within their pinned constant of the same model: of each other within the sum."""
    rs = np.random.RandomState(M + 1)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    uz = UniformChannelizer(FS, M, D, h, max_in=1 << 14)
    cz = Channelizer(FS, D, h, uz.freqs_hz, max_in=1 << 14)
    assert np.array_equal(uz.words, cz.words)
    worst = 0.0
    for out_base in (0, (1 << 40) // D + 3):
        nout = 2 * uz.info()[0] + 5
        in_base, n = uz.needed_input(out_base, nout)
        x = noise(rs, n)
        a = uz.process(in_base, x, out_base, nout)
        b = cz.process(in_base, x, out_base, nout)
        _, S = uz.model(in_base, x, out_base, nout)
        d = np.maximum(np.abs(a.real - b.real), np.abs(a.imag - b.imag))
        worst = max(worst, float((d / (EPS * S)).max()))
    uz.close()
    cz.close()
    print(f'M {M} D {D} T {T}: uniform against direct, worst {worst:.2f} * 2^-24 S (allowed {C_BOUND + DIRECT_C_BOUND})')
    assert worst <= C_BOUND + DIRECT_C_BOUND


def test_every_misuse_is_an_error_code():
    import torch
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    M, D, T = 16, 4, 9
    taps = np.linspace(0.1, 0.9, T).astype(np.float32)
    sel = np.array([3, 15], dtype=np.int32)
    words = np.array([1 << 60, 0], dtype=np.uint64)
    dev = torch.zeros(4096, dtype=torch.complex64, device='cuda')
    out = np.empty((2, 1024), np.complex64)
    hp = C.c_void_p()

    def params(**kw):
        d = dict(in_base=0, out_base=0, device_input=dev.data_ptr(), in_count=4096, out_count=1000, input=2, buffer=0)
        d.update(kw)
        return _lib.ChannelizerParams(**d)

    def plan(h, decim=D, t=taps, nt=T, b=sel, ns=2, fmt=0, scale=1.0):
        return lib.mfb_channelizer_set_plan_uniform(h, decim, t.ctypes.data if t is not None else None, nt,
                                                    b.ctypes.data if b is not None else None, ns, fmt, scale)

    def good(h):
        """The handle still works."""
        assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
        assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK

    def create(*a):
        return lib.mfb_channelizer_create_uniform(C.byref(hp), 0, *a)

    # create
    assert lib.mfb_channelizer_create_uniform(None, 0, 16, 1, 1, 1, 1) == ARG
    for a in ((0, 1, 1, 1, 1), (16, 0, 1, 1, 1), (16, 1, 0, 1, 1), (16, 1, 1, 0, 1), (16, 1, 1, 1, 0)):
        assert create(*a) == ARG and not hp.value
    for a in ((4, 1, 1, 1, 1), (24, 1, 1, 1, 1), (512, 1, 1, 1, 1), (16, 17, 1, 1, 1), (16, 1, 4097, 1, 1), (16, 1, 1, (1 << 24) + 1, 1),
              (16, 1, 1, 1, (1 << 22) + 1), (64, 33, 1, 1, 1 << 21), (256, 17, 1, 1, 1 << 22)):      # the last two: selected * max_out > 2^26
        assert create(*a) == UNSUP and not hp.value
    assert lib.mfb_channelizer_create_uniform(C.byref(hp), 1 << 20, 16, 1, 1, 1, 1) == ARG

    h = C.c_void_p()
    assert lib.mfb_channelizer_create_uniform(C.byref(h), 0, M, 4, 64, 4096, 1024) == OK
    # before a plan
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE
    assert lib.mfb_channelizer_info(h, None, None) == STATE
    assert lib.mfb_channelizer_end(h, None) == STATE
    assert lib.mfb_channelizer_input_buffer(h, 0, C.byref(hp), None) == STATE
    # the other kinds of plan on this handle, and this kind on an ordinary handle
    assert lib.mfb_channelizer_set_plan(h, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == STATE
    assert lib.mfb_channelizer_set_plan_rational(h, 3, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == STATE
    plain = C.c_void_p()
    assert lib.mfb_channelizer_create(C.byref(plain), 0, 4, 64, 4096, 1024) == OK
    assert plan(plain) == STATE
    assert lib.mfb_channelizer_set_plan(plain, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == OK
    assert plan(plain) == STATE
    good(plain)
    assert lib.mfb_channelizer_destroy(plain) == OK
    # set_plan_uniform
    assert plan(None) == ARG and plan(h, t=None) == ARG and plan(h, b=None) == ARG
    assert plan(h, nt=0) == ARG and plan(h, ns=0) == ARG
    assert plan(h, fmt=3) == ARG
    assert plan(h, fmt=1, scale=0.3) == ARG and plan(h, fmt=2, scale=-0.5) == ARG and plan(h, fmt=1, scale=float('inf')) == ARG
    for bad in (np.nan, np.inf):
        t2 = taps.copy()
        t2[3] = bad
        assert plan(h, t=t2) == ARG
    assert plan(h, t=np.ones(65, np.float32), nt=65) == ARG                  # more than the handle was created for
    assert plan(h, b=np.arange(5, dtype=np.int32), ns=5) == ARG
    for b in ([3, 16], [-1, 3], [3, 3]):                                     # outside [0, M), named twice
        assert plan(h, b=np.array(b, dtype=np.int32)) == ARG
    for decim in (1, 0, 17):
        assert plan(h, decim=decim) == UNSUP
    assert plan(h, t=np.ones(4097, np.float32), nt=4097) == UNSUP
    assert plan(h, b=np.arange(17, dtype=np.int32), ns=17) == UNSUP
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE          # every refusal left the handle without a plan
    assert plan(h, decim=16) == OK                                           # critical sampling
    assert plan(h) == OK
    fpw, cap = C.c_int(), C.c_int()
    assert lib.mfb_channelizer_info(h, C.byref(fpw), C.byref(cap)) == OK and fpw.value == 128 and cap.value == 64
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
    ptr, cnt, ms = C.c_void_p(), C.c_int64(), C.c_float()
    assert lib.mfb_channelizer_device_output(h, 1, 0, C.byref(ptr), C.byref(cnt)) == STATE      # set 1 was never written
    assert lib.mfb_channelizer_device_output(h, 0, 2, C.byref(ptr), C.byref(cnt)) == STATE      # two bins are selected
    assert lib.mfb_channelizer_device_output(h, 0, -1, C.byref(ptr), C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 2, 0, C.byref(ptr), C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 0, 0, None, C.byref(cnt)) == ARG
    assert lib.mfb_channelizer_device_output(h, 0, 1, C.byref(ptr), C.byref(cnt)) == OK and cnt.value == 1000 and ptr.value % 16 == 0
    assert lib.mfb_channelizer_elapsed_ms(h, C.byref(ms)) == OK and ms.value > 0
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
    taps = design_taps(16)

    def cycle():
        uz = UniformChannelizer(FS, 64, 16, taps, bins=[1, 63, 7, 32], sample_format='sc16', sample_scale=2.0 ** -15, max_in=n, max_out=n // 4)
        uz.process(0, x, 0, n // 16 - 16)
        uz.close()
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
