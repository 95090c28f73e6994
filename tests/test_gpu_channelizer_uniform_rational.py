"""Rational resampling on the raster on the device (csrc/channelize_uniform_rational_kernels.hpp,
mfb_uniform_channelizer_set_plan_rational) against its contract: within the derived bound of the float64 model
(``UniformChannelizer.model``, which is ``Channelizer._model_rational`` on the exact raster words), a pure function of the absolute
position bit for bit whatever the cut, the window, the output set and the selection, the integer uniform kernel's bits at U = 1, a
tone's phase advance that shares nothing with the model, and an error code for every misuse.

The error bound.  Per component |device - model| <= c * 2^-24 * S_m with S_m = sum_j |h[r + jU]| |x[q - j]|: a branch sum is a chain
of at most ceil(Tb / M) fused multiply-adds, Tb = ceil(T / U), followed by the unchanged transform of the uniform kernel, at most
3 u per bit of M, and 2 for the second order (tests/test_gpu_channelizer_uniform.py has the count per pass).  So
c <= ceil(Tb / M) + 3 log2 M + 2, asserted by every case for its own shape, and C_BOUND pins the constant that
tests/test_gpu_channelizer_uniform.py pins for the same arithmetic (profiles/channelizer_uniform_rational.md has the worst measured c
per shape)."""
import ctypes as C

import numpy as np
import pytest

import chur_shapes as cs
from pycusdr_amd import _lib
from pycusdr_amd.channelizer import UniformChannelizer, design_taps

pytestmark = pytest.mark.gpu

FS = 1.024e6
EPS = 2.0 ** -24
C_BOUND = 4                       # the pin of tests/test_gpu_channelizer_uniform.py
SHAPES = cs.SHAPES


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


CASES = [(s, far, 'cf32') for s in SHAPES for far in (False, True)]
CASES += [(SHAPES[1], False, 'sc16'), (SHAPES[1], True, 'sc8'), (SHAPES[3], True, 'sc16'), (SHAPES[3], False, 'sc8')]
WORST = {}


@pytest.mark.parametrize('case', range(len(CASES)))
def test_device_within_the_derived_bound_of_the_model(case):
    """Every shape from out_base 0 (zeros below position 0) and from an out_base with out_base * D > 2^40 (64-bit positions, the
    shift modulo M), two workgroups and a ragged tail; sc16 and sc8 also bit-equal to cf32 on the converted samples."""
    (M, U, D, T), far, fmt = CASES[case]
    rs = np.random.RandomState(900 + case)
    h = cs.taps_of(rs, U, D, T)
    sel = spread(M)
    out_base = ((1 << 40) // D + 3) if far else 0
    assert not far or out_base * D > 1 << 40
    uz = UniformChannelizer(FS, M, D, h, bins=sel, sample_format=fmt, sample_scale=scale_of(fmt), max_in=1 << 17, interp=U)
    F, cap = uz.info()
    assert cap == uz.Tb == -(-T // U) and F == cs.plan_frames(M, U, D, T) and F * M % 256 == 0
    nout = 2 * F + 5
    in_base, in_count = uz.needed_input(out_base, nout)
    assert in_count <= 1 << 17 and (in_base > 0) == far
    x = noise(rs, in_count, fmt)
    y = uz.process(in_base, x, out_base, nout)
    ref, S = uz.model(in_base, x, out_base, nout)
    uz.close()
    assert y.shape == ref.shape == (len(sel), nout) and S.min() > 0           # no output is left out of the comparison
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    c = float((err / (EPS * S)).max())
    WORST[(M, U, D, T)] = max(WORST.get((M, U, D, T), 0.0), c)
    print(f'case {case}: M {M} U {U} D {D} T {T} F {F} lds {cs.lds_bytes(M, U, D, T, F)} {fmt} out_base {out_base}: worst c = {c:.2f} '
          f'(ceiling {cs.ceiling(M, U, T)}); worst per shape so far {dict(sorted(WORST.items()))}')
    assert c <= cs.ceiling(M, U, T)
    assert c <= C_BOUND
    if fmt != 'cf32':
        f = x.astype(np.float32) * np.float32(scale_of(fmt))
        fz = UniformChannelizer(FS, M, D, h, bins=sel, max_in=1 << 17, interp=U)
        yf = fz.process(in_base, (f[:, 0] + 1j * f[:, 1]).astype(np.complex64), out_base, nout)
        fz.close()
        assert np.array_equal(bits(y), bits(yf))


@pytest.mark.parametrize('M, U, D, T', [SHAPES[1], SHAPES[3]])
def test_pure_function_of_position(M, U, D, T):
    """One span computed whole equals the same span in pieces whose cuts are multiples of neither U nor F, from input windows with
    odd and even in_base and a wider one, in either output set, and with a subset selection, one bin and signed indices against
    the rows of the full one: bit for bit."""
    rs = np.random.RandomState(M + U)
    h = cs.taps_of(rs, U, D, T)
    every = UniformChannelizer(FS, M, D, h, max_in=1 << 17, interp=U)
    F, _ = every.info()
    base = 1001
    counts, at = [], 0
    for n in (1, F - 2, F + U + 1, 2 * F + 7, U + 2, 3):     # each piece lengthened until its end is a multiple of neither
        while (at + n) % U == 0 or (at + n) % F == 0 or (base + at + n) % U == 0 or (base + at + n) % F == 0:
            n += 1
        counts.append(n)
        at += n
    counts.append(41)
    cuts = np.cumsum(counts)[:-1]
    assert all(c % U and c % F and (base + c) % U and (base + c) % F for c in cuts) and len(counts) == 7
    assert any(n < F for n in counts) and any(n > 2 * F for n in counts)
    nout = sum(counts)
    in_base, in_count = every.needed_input(base, nout)
    x = noise(rs, in_count)
    whole = every.process(in_base, x, base, nout)
    assert whole.shape == (M, nout) and np.abs(whole).min() > 0
    subset = [M - 3, 2, M // 2, 0, M - 1, 1]
    signed = [-3, 2, -(M // 2), 0, -1, 1]
    one = UniformChannelizer(FS, M, D, h, bins=[M - 3], max_in=1 << 17, interp=U)
    some = UniformChannelizer(FS, M, D, h, bins=subset, max_in=1 << 17, interp=U)
    neg = UniformChannelizer(FS, M, D, h, bins=signed, max_in=1 << 17, interp=U)
    assert one.info() == some.info() == neg.info() == every.info()
    assert np.array_equal(bits(one.process(in_base, x, base, nout)), bits(whole[[M - 3]]))
    assert np.array_equal(bits(some.process(in_base, x, base, nout)), bits(whole[subset]))
    assert np.array_equal(bits(neg.process(in_base, x, base, nout)), bits(whole[subset]))
    parities, wider, at = set(), 0, base
    for i, n in enumerate(counts):
        b, c = every.needed_input(at, n)
        if i % 3 == 2 and b > in_base:                       # a wider window than needed: one sample earlier, two later
            b, c = b - 1, min(c + 3, in_base + in_count - b + 1)
            wider += 1
        parities.add(b & 1)
        want = whole[:, at - base:at - base + n]
        win = x[b - in_base:b - in_base + c]
        assert np.array_equal(bits(every.process(b, win, at, n, buffer=i & 1)), bits(want)), (i, n)
        assert np.array_equal(bits(some.process(b, win, at, n, buffer=(i & 1) ^ 1)), bits(want[subset])), (i, n)
        assert np.array_equal(bits(one.process(b, win, at, n)), bits(want[[M - 3]])), (i, n)
        at += n
    assert at == base + nout and parities == {0, 1} and wider >= 2
    for z in (every, one, some, neg):
        z.close()


@pytest.mark.parametrize('M, U, D, T, Z', [(8, 3, 16, 100, 64), (16, 2, 31, 257, 496)])
def test_positions_below_zero_read_zeros(M, U, D, T, Z):
    """The stream x at out_base 0 equals the stream [Z zeros, x] at out_base Z U / D, Z a multiple of lcm(D, M): q moves by Z, r
    and every bin's phase stay.  Outputs that read nothing but zeros are zero exactly."""
    rs = np.random.RandomState(2)
    assert Z % D == 0 and Z % M == 0
    h = cs.taps_of(rs, U, D, T)
    x = noise(rs, 4300)
    uz = UniformChannelizer(FS, M, D, h, max_in=8192, interp=U)
    nout = 270
    assert uz.needed_input(0, nout)[1] <= len(x)
    a = uz.process(0, x, 0, nout)
    b = uz.process(0, np.r_[np.zeros(Z, np.complex64), x], Z * U // D, nout)
    ref, S = uz.model(0, x, 0, nout)
    assert np.array_equal(bits(a), bits(b))
    assert np.all(np.maximum(np.abs(a.real - ref.real), np.abs(a.imag - ref.imag)) <= cs.ceiling(M, U, T) * EPS * S)
    # frame 0 (q = 0, r = 0) holds one value and zeros, which every addition passes on exactly: bin 0's first output is that product
    assert a[0, 0] == np.complex64(complex(h[0] * x[0].real, h[0] * x[0].imag))
    # S_m = 0: the first `quiet` outputs of [Z zeros, x] read zeros only
    quiet = Z * U // D
    zeros, Sz = uz.model(0, np.r_[np.zeros(Z, np.complex64), x], 0, quiet)
    z = uz.process(0, np.r_[np.zeros(Z, np.complex64), x], 0, quiet)
    uz.close()
    assert quiet >= 12 and np.all(Sz == 0) and np.all(z == 0)


@pytest.mark.parametrize('M, D, T', [(8, 3, 37), (64, 48, 1025), (256, 128, 257)])
def test_interp_1_through_the_rational_kernel_gives_the_integer_kernels_bits(M, D, T):
    rs = np.random.RandomState(M + D)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    a = UniformChannelizer(FS, M, D, h, max_in=1 << 17, force_rational=True)
    b = UniformChannelizer(FS, M, D, h, max_in=1 << 17)
    assert a.rational and not b.rational and a.info() == b.info()
    F = a.info()[0]
    for out_base in (0, 1001, (1 << 40) // D + 3):
        nout = 2 * F + 5
        in_base, n = a.needed_input(out_base, nout)
        assert (in_base, n) == b.needed_input(out_base, nout)
        x = noise(rs, n)
        ya, yb = a.process(in_base, x, out_base, nout), b.process(in_base, x, out_base, nout)
        assert np.abs(yb).min() > 0 and np.array_equal(bits(ya), bits(yb)), out_base
    a.close()
    b.close()


def test_a_tone_advances_by_its_offset_per_output():
    """x[n] = exp(2 pi i w n / 2^20) with w = b 2^20 / M + a: a tone ``a / 2^20`` cycles per sample above the centre of bin b.
    Outputs U apart share the branch r and read inputs exactly D apart, so far from position 0
    y_b[m + U] = y_b[m] exp(2 pi i a D / 2^20) whatever the taps: the phase of every residue class of m advances
    2 pi a D / (2^20 U) per output.  A least-squares line through n points U apart whose phases are each off by at most e has a slope
    off by at most e sum|i - mean| / (U sum (i - mean)^2); e = sqrt(2) (c + 1) 2^-24 S / |y| with c the ceiling and the 1 for the
    rounding of the tone's own samples to complex64.  Nothing here touches the model."""
    M, U, D = 64, 8, 125
    h = design_taps(D, interp=U)
    T = len(h)
    b, a = 5, 1049                                            # a D / 2^20 = 0.125 turns per U outputs, well inside the pass band
    w = b * (1 << 20) // M + a
    uz = UniformChannelizer(FS, M, D, h, bins=[b, M - b], max_in=1 << 17, interp=U)
    F = uz.info()[0]
    out_base, nout = 5 * T, 4 * F + 5
    in_base, n = uz.needed_input(out_base, nout)
    assert in_base > 0
    pos = np.arange(in_base, in_base + n, dtype=np.int64)
    x = np.exp(2j * np.pi * ((w * pos) % (1 << 20)) / (1 << 20)).astype(np.complex64)
    y = uz.process(in_base, x, out_base, nout)
    uz.close()
    want = 2 * np.pi * a * D / ((1 << 20) * U)
    c = cs.ceiling(M, U, T)
    worst = 0.0
    for cls in range(U):
        m = np.arange(cls, nout, U)
        r = ((out_base + cls) * D) % U
        S = np.abs(h[r::U].astype(np.float64)).sum()
        yc = y[0, m]
        assert np.abs(yc).min() > 0.9                         # in the pass band: about unit gain
        e = np.sqrt(2) * (c + 1) * EPS * S / np.abs(yc).min()
        i = np.arange(len(m), dtype=np.float64)
        slope = np.polyfit(i * U, np.unwrap(np.angle(yc.astype(np.complex128))), 1)[0]
        allowed = e * np.abs(i - i.mean()).sum() / (U * ((i - i.mean()) ** 2).sum())
        worst = max(worst, abs(slope - want) / allowed)
        print(f'class {cls} (r = {r}, {len(m)} points): slope {slope:.9f} rad per output, expected {want:.9f}, off by '
              f'{abs(slope - want):.2e} of {allowed:.2e} allowed')
        assert abs(slope - want) <= allowed, cls
    assert np.abs(y[1]).max() < 1e-3                          # the mirror bin: deep in the stop band


def test_the_state_machine():
    import torch
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    M, U, D, T = 16, 3, 8, 20
    taps = np.linspace(0.1, 0.9, T).astype(np.float32)
    sel = np.array([3, 15], dtype=np.int32)
    words = np.array([1 << 60, 0], dtype=np.uint64)
    dev = torch.zeros(4096, dtype=torch.complex64, device='cuda')
    out = np.empty((2, 1024), np.complex64)

    def params(**kw):
        d = dict(in_base=0, out_base=0, device_input=dev.data_ptr(), in_count=4096, out_count=1000, input=2, buffer=0)
        d.update(kw)
        return _lib.ChannelizerParams(**d)

    def plan(h, interp=U, decim=D, t=taps, nt=T, b=sel, ns=2, fmt=0, scale=1.0):
        return lib.mfb_uniform_channelizer_set_plan_rational(h, interp, decim, t.ctypes.data if t is not None else None, nt,
                                                             b.ctypes.data if b is not None else None, ns, fmt, scale)

    def integer_plan(h):
        return lib.mfb_channelizer_set_plan_uniform(h, D, taps.ctypes.data, 16, sel.ctypes.data, 2, 0, 1.0)

    def good(h):
        """The handle still works."""
        assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
        assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK

    h = C.c_void_p()
    assert lib.mfb_channelizer_create_uniform(C.byref(h), 0, M, 4, 16, 4096, 1024) == OK          # 16 taps per branch
    # plan kinds do not mix
    plain = C.c_void_p()
    assert lib.mfb_channelizer_create(C.byref(plain), 0, 4, 64, 4096, 1024) == OK
    assert plan(plain) == STATE
    assert lib.mfb_channelizer_set_plan_rational(plain, U, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == OK
    assert plan(plain) == STATE
    good(plain)
    assert lib.mfb_channelizer_destroy(plain) == OK
    assert lib.mfb_channelizer_set_plan(h, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == STATE
    assert lib.mfb_channelizer_set_plan_rational(h, U, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == STATE
    # the limits
    for kw in (dict(interp=0), dict(interp=-1), dict(interp=33, decim=35, t=np.ones(40, np.float32), nt=40), dict(decim=49), dict(decim=1),
               dict(interp=1, decim=17), dict(b=np.arange(17, dtype=np.int32), ns=17)):
        assert plan(h, **kw) == UNSUP, kw
    big = np.ones(3 * 4096 + 1, np.float32)
    assert plan(h, t=big, nt=len(big)) == UNSUP                                                 # ceil(T / U) > 4096
    # the arguments
    for kw in (dict(decim=6), dict(interp=4, decim=6), dict(decim=3), dict(decim=2), dict(interp=5, decim=4), dict(nt=2),
               dict(t=np.ones(49, np.float32), nt=49),                                          # 17 taps per branch: more than the handle's
               dict(b=np.array([3, 16], np.int32)), dict(b=np.array([-1, 3], np.int32)), dict(b=np.array([3, 3], np.int32)),
               dict(b=np.arange(5, dtype=np.int32), ns=5), dict(fmt=3), dict(fmt=1, scale=0.3), dict(t=None), dict(b=None), dict(nt=0),
               dict(ns=0)):
        assert plan(h, **kw) == ARG, kw
    bad = taps.copy()
    bad[3] = np.nan
    assert plan(h, t=bad) == ARG and plan(None) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == STATE          # every refusal left the handle without a plan
    assert plan(h, t=np.ones(48, np.float32), nt=48) == OK                   # 16 taps per branch: the handle's capacity
    assert plan(h, decim=47) == OK                                           # D = U M - 1
    assert plan(h, interp=1, decim=16, nt=16) == OK                          # the rational kernel at U = 1, critical sampling
    assert plan(h) == OK
    fpw, cap = C.c_int(), C.c_int()
    assert lib.mfb_channelizer_info(h, C.byref(fpw), C.byref(cap)) == OK
    assert fpw.value == cs.plan_frames(M, U, D, T) == 128 and cap.value == 16
    good(h)
    # the input rule of a rational plan, one sample short at either end: outputs 100 .. 299 read inputs
    # q(100) - (Tb - 1) = 266 - 6 = 260 .. q(299) = 797
    need = dict(out_base=100, out_count=200)
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=260, in_count=538, **need))) == OK
    assert lib.mfb_channelizer_end(h, None) == OK
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=261, in_count=537, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(in_base=260, in_count=537, **need))) == ARG
    assert lib.mfb_channelizer_begin(h, C.byref(params(out_base=(1 << 62) // D))) == UNSUP
    # the survey stays with integer plans
    assert lib.mfb_channelizer_set_survey(h, 8, 4, 4.0) == UNSUP
    assert lib.mfb_channelizer_set_survey(h, 0, 0, 1.0) == UNSUP
    assert lib.mfb_channelizer_survey_begin(h, C.byref(params(out_count=992)), 1) == STATE
    good(h)
    assert integer_plan(h) == OK
    assert lib.mfb_channelizer_set_survey(h, 8, 4, 4.0) == OK
    assert plan(h) == UNSUP                                                  # a survey is set
    assert lib.mfb_channelizer_survey_begin(h, C.byref(params(out_count=504)), 1) == OK          # and the integer plan is still in force
    assert lib.mfb_channelizer_survey_end(h, None, None, None, None) == OK
    assert lib.mfb_channelizer_set_survey(h, 0, 0, 1.0) == OK
    assert plan(h) == OK
    # a plan while a call is in flight
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
    assert plan(h) == STATE and integer_plan(h) == STATE
    assert lib.mfb_channelizer_begin(h, C.byref(params(buffer=1))) == STATE
    assert lib.mfb_channelizer_end(h, out.ctypes.data) == OK
    ptr, cnt, ms = C.c_void_p(), C.c_int64(), C.c_float()
    assert lib.mfb_channelizer_device_output(h, 0, 1, C.byref(ptr), C.byref(cnt)) == OK and cnt.value == 1000 and ptr.value % 16 == 0
    assert lib.mfb_channelizer_elapsed_ms(h, C.byref(ms)) == OK and ms.value > 0
    good(h)
    assert lib.mfb_channelizer_destroy(h) == OK
    # the Python surface says the same
    uz = UniformChannelizer(FS, M, D, taps, bins=[3, 15], max_in=4096, interp=U)
    with pytest.raises(ValueError, match='rational'):
        uz.set_survey(8)
    uz.close()
