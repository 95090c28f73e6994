"""The synthesiser on the device (mfb_synthesizer_*, csrc/synthesize_uniform_kernels.hpp) against the float64 model of
pycusdr_amd/synthesizer.py: the derived error bound on every shape from two bases, purity under cuts, zero streams, host and device
sources, every misuse as a status code, device memory over create / destroy cycles, and the round trip through the uniform
channeliser on the device."""
import ctypes as C

import numpy as np
import pytest

import synth_scenes as sc
from pycusdr_amd import _lib
from pycusdr_amd.channelizer import UniformChannelizer
from pycusdr_amd.synthesizer import UniformSynthesizer, frames_per_workgroup, pack_placements

pytestmark = pytest.mark.gpu

EPS = sc.EPS
C_BOUND = 4                       # twice the worst measured c (1.81, M = 32, I = 32, T = 32 from out_base 2^40 + 3), rounded up


def _copy_to_host(dst, dev_ptr):
    """hipMemcpy of the process's one HIP runtime (pycusdr_amd._lib loads it globally before the library)."""
    fn = C.CDLL(None).hipMemcpy
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    assert fn(dst.ctypes.data, dev_ptr, dst.nbytes, 2) == 0  # hipMemcpyDeviceToHost


SHAPES = [(8, 8, 1), (8, 2, 8), (8, 3, 37), (16, 16, 129), (16, 5, 17), (32, 32, 32), (32, 7, 33), (64, 16, 257), (64, 48, 769),
          (128, 96, 1537), (256, 256, 4096), (256, 128, 257), (256, 2, 33)]
CASES = [(s, base) for s in SHAPES for base in (0, (1 << 40) + 3)]
WORST = {}


@pytest.mark.parametrize('case', range(len(CASES)))
def test_device_within_the_derived_bound_of_the_model(case):
    (M, I, T), out_base = CASES[case]
    rs = np.random.RandomState(700 + case)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    s = UniformSynthesizer(sc.FS, M, I, h, max_out=1 << 16, max_source=1 << 16, max_frames=64)
    F, R = s.info()
    J = -(-T // I)
    assert F == frames_per_workgroup(M, I, T) >= 1 and R == F + J - 1
    nout = 2 * F * I + 5
    first, count = s.needed_frames(out_base, nout)
    bins = sc.spread(M)
    pl, need = sc.two_per_bin(s, bins, first, count)
    assert (pl[0].start < first) == (out_base > 0) and pl[0].start + pl[0].length == pl[1].start       # before the reach; abutting
    assert pl[2].start + pl[2].length < pl[3].start and {p.gain for p in pl} == {1.0, float(np.float32(0.37))}
    s.set_source(sc.noise(rs, need))
    w = s.process(out_base, nout, pl)
    ref, S = s.model(out_base, nout, pl)
    s.close()
    assert w.shape == ref.shape == S.shape == (nout,)
    has_taps = (out_base + np.arange(nout)) % I < T          # (T < I: the other outputs have no tap and are exactly zero)
    assert has_taps.all() or T < I
    assert S[has_taps].min() > 0                             # no output is left out of the comparison
    assert not w[~has_taps].any() and not ref[~has_taps].any()
    err = np.maximum(np.abs(w.real - ref.real), np.abs(w.imag - ref.imag))[has_taps]
    c = float((err / (EPS * S[has_taps])).max())
    WORST[(M, T)] = max(WORST.get((M, T), 0.0), c)
    print(f'case {case}: M {M} I {I} T {T} F {F} out_base {out_base}: worst c = {c:.2f} (ceiling {sc.ceiling(M, I, T)}); '
          f'worst per (M, T) so far {dict(sorted(WORST.items()))}')
    assert c <= sc.ceiling(M, I, T)
    assert c <= C_BOUND


@pytest.mark.parametrize('M, I, T', [(32, 7, 33), (64, 64, 200)])
def test_pure_function_of_position(M, I, T):
    """One span computed whole equals the same span in uneven chunks around F I, in either output set, fetched by copy or from
    the output set on the device: bit for bit."""
    rs = np.random.RandomState(M)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    s = UniformSynthesizer(sc.FS, M, I, h, max_out=1 << 16, max_source=1 << 16, max_frames=64)
    F, _ = s.info()
    base = 1001
    counts = (1, F * I - 1, F * I, F * I + 1, 2 * F * I + 7, 3, I - 1, 40)
    nout = sum(counts)
    first, count = s.needed_frames(base, nout)
    pl, need = sc.two_per_bin(s, sc.spread(M), first, count)
    s.set_source(sc.noise(rs, need))
    whole = s.process(base, nout, pl)
    assert np.abs(whole).min() > 0
    at = base
    for i, n in enumerate(counts):
        want = whole[at - base:at - base + n]
        assert np.array_equal(sc.bits(s.process(at, n, pl, buffer=i & 1)), sc.bits(want)), (i, n)
        assert s.process(at, n, pl[::-1], copy=False, buffer=(i & 1) ^ 1) is None          # the order of the list does not matter
        ptr, cnt = s.device_output((i & 1) ^ 1)
        assert cnt == n and ptr % 16 == 0
        got = np.empty(n, np.complex64)
        _copy_to_host(got, ptr)
        assert np.array_equal(sc.bits(got), sc.bits(want)), (i, n)
        at += n
    assert at == base + nout
    s.close()


def test_zero_streams_and_unreached_outputs():
    M, I, T = 16, 5, 17
    rs = np.random.RandomState(5)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    s = UniformSynthesizer(sc.FS, M, I, h, max_out=1 << 14, max_source=1 << 14)
    src = sc.noise(rs, 400)
    src[200:] = 0                                            # the samples of the extra placement
    s.set_source(src)
    J = s.J
    pl = [s.placement(3, 50, 0, 60), s.placement(-2, 70, 60, 30, 0.37)]
    nout = 200 * I
    plain = s.process(0, nout, pl)
    extra = s.process(0, nout, pl + [s.placement(9, 0, 200, 200, 0.37)])
    assert np.array_equal(plain, extra)                      # as values: -0 equals +0
    ref, S = s.model(0, nout, pl)
    reached = S > 0
    q, r = np.divmod(np.arange(nout), I)                     # reached: a tap r + j I < T stands on a frame 50 <= q - j < 110
    assert np.array_equal(reached, np.any([(r + j * I < T) & (q - j >= 50) & (q - j < 110) for j in range(J)], axis=0))
    assert reached[50 * I] and not reached[50 * I - 1] and reached[(109 + J - 1) * I] and not reached[(109 + J - 1) * I + 2]
    assert not plain[~reached].any() and np.abs(plain[reached]).min() > 0
    assert not s.process(0, 49 * I, pl).any() and not s.process(0, 100, []).any()
    s.close()


def test_host_source_equals_device_source():
    """a DeviceBatch from the modulator, used in place, against its samples copied to the host and back"""
    from pycusdr_amd import config as cfg
    from pycusdr_amd.modulator import Modulator
    from pycusdr_amd.protocol import loadProtocol
    conf = cfg.cc11xx_config(blockSize=14, doppCarrierSteps=64, samplesPerSym=16)
    p = loadProtocol('CC11xx')(conf=conf)
    tx = Modulator(conf, conf['Radios']['Rx']['UHF-H'], p, backend='hip')
    tx.set_rangerate(0.0)
    batch = tx.modulate_device([tx.encodeAndFrame(np.arange(1, 21, dtype=np.uint8)), tx.encodeAndFrame(np.arange(50, 20, -1).astype(np.uint8))])
    host = np.empty(batch.total, np.complex64)
    _copy_to_host(host, batch.ptr)
    assert np.abs(host).max() > 0.5
    M, I = 8, 4
    h = (4 * np.hanning(33) / np.hanning(33).sum()).astype(np.float32)
    out = []
    for source in (batch, host):
        s = UniformSynthesizer(sc.FS, M, I, h, max_out=1 << 18, max_source=1 << 18)
        s.set_source(source)
        assert s.source_len == batch.total
        pl = [s.placement(2, 10, int(batch.sample_off[0]), batch.frame_len(0)), s.placement(6, 300, int(batch.sample_off[1]), batch.frame_len(1), 0.37)]
        nout = min(1 << 18, I * (max(batch.frame_len(0), batch.frame_len(1)) + 400))
        out.append(s.process(0, nout, pl))
        s.close()
    tx.close()
    assert np.array_equal(sc.bits(out[0]), sc.bits(out[1])) and np.abs(out[0]).max() > 0.1 * np.abs(host).max()


def _hip(name, *argtypes):
    fn = getattr(C.CDLL(None), name)
    fn.argtypes, fn.restype = list(argtypes), C.c_int
    return fn


def _device_free():
    """free bytes of the device, everything queued finished"""
    free, total = C.c_size_t(), C.c_size_t()
    assert _hip('hipDeviceSynchronize')() == 0
    assert _hip('hipMemGetInfo', C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))(C.byref(free), C.byref(total)) == 0
    return free.value


def test_every_misuse_is_an_error_code():
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    M, I, T = 16, 4, 9
    taps = np.linspace(0.1, 0.9, T).astype(np.float32)
    feeder = UniformSynthesizer(sc.FS, 8, 2, np.ones(2, np.float32), max_out=4096, max_source=16)      # device memory: its output set
    feeder.set_source(np.ones(16, np.complex64))
    feeder.process(0, 4096, [feeder.placement(0, 0, 0, 16)], copy=False, buffer=0)
    dev_ptr, dev_n = feeder.device_output(0)
    assert dev_n == 4096
    host = np.ones(1000, np.complex64)
    out = np.full(1024, 7, np.complex64)
    hp = C.c_void_p()

    def params(**kw):
        d = dict(out_base=0, out_count=1000, buffer=0)
        d.update(kw)
        return _lib.SynthesizerParams(**d)

    class P:
        def __init__(self, bin=1, start=0, src=0, length=10, gain=1.0):
            self.bin, self.start, self.src, self.length, self.gain = bin, start, src, length, gain

    def begin(h, pl, **kw):
        a = pack_placements(pl)
        return lib.mfb_synthesizer_begin(h, C.byref(params(**kw)), a.ctypes.data if len(a) else None, len(a))

    def good(h):
        """The handle still works, and nothing stayed in flight."""
        assert begin(h, [P()]) == OK
        assert lib.mfb_synthesizer_end(h, out.ctypes.data) == OK

    def create(*a):
        return lib.mfb_synthesizer_create(C.byref(hp), 0, *a)

    def plan(h, interp=I, t=taps, nt=T):
        return lib.mfb_synthesizer_set_plan(h, interp, t.ctypes.data if t is not None else None, nt)

    # create: (nbins, max_taps, max_out, max_source, max_frames)
    assert lib.mfb_synthesizer_create(None, 0, 16, 1, 1, 1, 1) == ARG
    for a in ((0, 1, 1, 1, 1), (16, 0, 1, 1, 1), (16, 1, 0, 1, 1), (16, 1, 1, 0, 1), (16, 1, 1, 1, 0)):
        assert create(*a) == ARG and not hp.value
    for a in ((4, 1, 1, 1, 1), (24, 1, 1, 1, 1), (512, 1, 1, 1, 1), (16, 4097, 1, 1, 1), (16, 1, (1 << 24) + 1, 1, 1), (16, 1, 1, (1 << 26) + 1, 1),
              (16, 1, 1, 1, 4097)):
        assert create(*a) == UNSUP and not hp.value
    assert lib.mfb_synthesizer_create(C.byref(hp), 1 << 20, 16, 1, 1, 1, 1) == ARG
    assert lib.mfb_synthesizer_destroy(None) == ARG

    h = C.c_void_p()
    assert lib.mfb_synthesizer_create(C.byref(h), 0, M, 64, 1024, 1000, 4) == OK
    # before a plan, before a source
    assert begin(h, [P()]) == STATE
    assert lib.mfb_synthesizer_info(h, None, None) == STATE
    assert lib.mfb_synthesizer_end(h, None) == STATE
    ms = C.c_float()
    assert lib.mfb_synthesizer_elapsed_ms(h, C.byref(ms)) == STATE
    # set_plan
    assert plan(None) == ARG and plan(h, t=None) == ARG and plan(h, nt=0) == ARG
    for bad in (np.nan, np.inf):
        t2 = taps.copy()
        t2[3] = bad
        assert plan(h, t=t2) == ARG
    assert plan(h, t=np.ones(65, np.float32), nt=65) == ARG                  # more than the handle was created for
    for interp in (1, 0, 17):
        assert plan(h, interp=interp) == UNSUP
    assert plan(h, t=np.ones(4097, np.float32), nt=4097) == UNSUP
    big, small = C.c_void_p(), C.c_void_p()
    assert lib.mfb_synthesizer_create(C.byref(big), 0, 8, 4096, 16, 16, 1) == OK
    assert lib.mfb_synthesizer_set_plan(big, 2, np.ones(4096, np.float32).ctypes.data, 4096) == UNSUP       # 2048 frames do not fit
    assert lib.mfb_synthesizer_set_plan(big, 8, np.ones(4096, np.float32).ctypes.data, 4096) == OK
    assert lib.mfb_synthesizer_destroy(big) == OK
    assert begin(h, [P()]) == STATE                                          # every refusal left the handle without a plan
    assert plan(h, interp=16) == OK                                          # I = M
    assert plan(h) == OK
    fpw, rows = C.c_int(), C.c_int()
    assert lib.mfb_synthesizer_info(h, C.byref(fpw), C.byref(rows)) == OK and fpw.value == 128 and rows.value == 130
    assert begin(h, [P()]) == STATE                                          # a plan, no source
    # set_source
    assert lib.mfb_synthesizer_set_source(None, host.ctypes.data, 1000, 0) == ARG
    assert lib.mfb_synthesizer_set_source(h, None, 1000, 0) == ARG
    assert lib.mfb_synthesizer_set_source(h, host.ctypes.data, 0, 0) == ARG
    assert lib.mfb_synthesizer_set_source(h, host.ctypes.data, 1001, 0) == ARG         # more than the handle was created for
    assert lib.mfb_synthesizer_set_source(h, dev_ptr + 4, 100, 1) == ARG
    assert begin(h, [P()]) == STATE
    assert lib.mfb_synthesizer_set_source(h, dev_ptr, 4096, 1) == OK            # device memory may be longer than max_source
    good(h)
    assert lib.mfb_synthesizer_set_source(h, host.ctypes.data, 1000, 0) == OK
    good(h)
    # begin: ARG
    assert lib.mfb_synthesizer_begin(None, C.byref(params()), None, 0) == ARG
    assert lib.mfb_synthesizer_begin(h, None, None, 0) == ARG
    assert lib.mfb_synthesizer_begin(h, C.byref(params()), None, 1) == ARG
    assert lib.mfb_synthesizer_begin(h, C.byref(params()), None, -1) == ARG
    for kw in (dict(out_count=0), dict(out_base=-1), dict(buffer=2), dict(buffer=-1), dict(out_count=1025)):
        assert begin(h, [P()], **kw) == ARG, kw
    for bad in ([P(start=-1)], [P(src=-1)], [P(length=0)], [P(length=-3)], [P(src=991)], [P(src=1000, length=1)], [P(bin=-1)], [P(bin=16)],
                [P(gain=np.inf)], [P(gain=np.nan)], [P(), P(start=9, src=10)], [P(start=20), P(bin=2), P(start=11, src=10)], [P(length=1)] * 5):
        assert begin(h, bad) == ARG, [vars(p) for p in bad]
    # begin: UNSUPPORTED
    assert begin(h, [P()], out_count=(1 << 24) + 1) == UNSUP
    assert begin(h, [P()], out_base=1 << 62) == UNSUP
    assert begin(h, [P(start=1 << 62)]) == UNSUP
    assert lib.mfb_synthesizer_begin(h, C.byref(params()), pack_placements([P()]).ctypes.data, 4097) == UNSUP
    assert lib.mfb_synthesizer_end(h, None) == STATE                         # none of them launched anything
    good(h)
    assert begin(h, [P(), P(start=10, src=10), P(bin=2)]) == OK              # abutting; the same span on another bin
    assert lib.mfb_synthesizer_end(h, None) == OK
    assert begin(h, []) == OK and lib.mfb_synthesizer_end(h, out.ctypes.data) == OK and not out[:1000].any() and out[1000] == 7
    # STATE
    ptr, cnt = C.c_void_p(), C.c_int64()
    assert lib.mfb_synthesizer_device_output(h, 1, C.byref(ptr), C.byref(cnt)) == STATE         # set 1 was never written
    assert lib.mfb_synthesizer_device_output(h, 2, C.byref(ptr), C.byref(cnt)) == ARG
    assert lib.mfb_synthesizer_device_output(h, 0, None, C.byref(cnt)) == ARG
    assert lib.mfb_synthesizer_device_output(h, 0, C.byref(ptr), C.byref(cnt)) == OK and cnt.value == 1000 and ptr.value % 16 == 0
    assert lib.mfb_synthesizer_elapsed_ms(h, None) == ARG
    assert lib.mfb_synthesizer_elapsed_ms(h, C.byref(ms)) == OK and ms.value > 0
    assert lib.mfb_synthesizer_end(h, None) == STATE
    assert begin(h, [P()]) == OK
    assert begin(h, [P()], buffer=1) == STATE
    assert plan(h) == STATE
    assert lib.mfb_synthesizer_set_source(h, host.ctypes.data, 1000, 0) == STATE
    assert lib.mfb_synthesizer_device_output(h, 0, C.byref(ptr), C.byref(cnt)) == STATE         # in flight
    assert lib.mfb_synthesizer_elapsed_ms(h, C.byref(ms)) == STATE
    assert lib.mfb_synthesizer_end(h, out.ctypes.data) == OK
    assert plan(h) == OK
    assert lib.mfb_synthesizer_device_output(h, 0, C.byref(ptr), C.byref(cnt)) == STATE         # what the set holds belongs to the plan before
    good(h)
    assert lib.mfb_synthesizer_destroy(h) == OK
    feeder.close()


def test_cycles_return_device_memory():
    rs = np.random.RandomState(9)
    n = 1 << 20
    x = sc.noise(rs, n // 16)
    taps = (16 * np.hanning(257) / np.hanning(257).sum()).astype(np.float32)

    def cycle():
        s = UniformSynthesizer(sc.FS, 64, 16, taps, max_out=n, max_source=n // 16)
        s.set_source(x)
        s.process(0, n, [s.placement(b, 0, 0, n // 16) for b in (1, 63, 7, 32)])
        s.close()
    assert 20 * 2 * n * 8 > (32 << 20)                       # the output sets alone would cross the bound
    for _ in range(2):
        cycle()
    free0 = _device_free()
    for _ in range(20):
        cycle()
    free1 = _device_free()
    print(f'20 cycles: device free {free0 >> 20} -> {free1 >> 20} MiB')
    assert abs(free0 - free1) < (32 << 20), (free0, free1)


def test_round_trip_on_the_device_within_the_two_bounds_of_the_model_round_trip():
    """The scene of tests/test_synthesizer_host.py: UniformSynthesizer('hip') -> UniformChannelizer('hip'), fed the synthesiser's
    device_output.  With w the synthesiser's model and y the channeliser's model of it, the device's y^ obeys
        |y^ - y| <= c_a u S_a[m] + sum_t |h_a[t]| |w^ - w|[m D - t],      |w^ - w|[n] <= sqrt(2) (c_s u S_s[n] + u |w[n]|)
    per component (the sqrt(2): a per-component bound on w^ as a modulus; u |w|: the model's w is handed on as complex64),
    c_a and c_s the two derived ceilings, S from the models."""
    h, g, x = sc.round_trip_scene()
    M, I, bins, nfr = sc.RT_M, sc.RT_I, list(sc.RT_BINS), sc.RT_FRAMES + sc.RT_DELAY
    nw = nfr * I
    s = UniformSynthesizer(sc.FS, M, I, g, max_out=nw, max_source=x.size)
    s.set_source(x.reshape(-1))
    pl = [s.placement(b, 0, k * sc.RT_FRAMES, sc.RT_FRAMES) for k, b in enumerate(bins)]
    assert s.process(0, nw, pl, copy=False, buffer=0) is None
    ptr, cnt = s.device_output(0)
    assert cnt == nw
    uz = UniformChannelizer(sc.FS, M, I, h, bins=bins, max_in=nw, max_out=nfr)
    y = uz.process(0, (ptr, nw), 0, nfr)
    w, Ss = s.model(0, nw, pl)
    ym, Sa = UniformChannelizer(sc.FS, M, I, h, bins=bins, backend='host').model(0, w, 0, nfr)
    uz.close()
    s.close()
    dw = np.sqrt(2) * EPS * (sc.ceiling(M, I, len(g)) * Ss + np.abs(w))
    T = len(h)
    padded = np.r_[np.zeros(T - 1), dw]
    through = np.lib.stride_tricks.sliding_window_view(padded, T)[::I][:nfr] @ np.abs(h[::-1].astype(np.float64))
    bound = sc.analysis_ceiling(M, T) * EPS * Sa + through
    err = np.maximum(np.abs(y.real - ym.real), np.abs(y.imag - ym.imag))
    live = bound > 0
    print(f'round trip on the device: worst error / bound = {float((err[:, live] / bound[live]).max()):.3f}; '
          f'worst deviation from the streams {np.abs(y[:, sc.RT_DELAY:] - x).max():.2e}')
    assert (err <= bound).all()
    assert np.abs(y[:, sc.RT_DELAY:] - x).max() <= 1e-3 * np.abs(x).max()
