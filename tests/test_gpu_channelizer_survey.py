"""The survey of the raster on the device (csrc/channelize_survey_kernels.hpp, mfb_channelizer_set_survey / _survey_begin /
_survey_end) against its contract: the power table is the numpy definition applied to the device's own outputs, floor and mask are
the definitions applied to that table, all of it a pure function of the position bit for bit, the written outputs untouched, within a
derived bound of the host back end, an error code for every misuse, and device memory returned.

Every shape runs at three cell lengths around the survey launch's frames per workgroup Fs (``survey_info()``): Fs / 2 (several cells
in a workgroup), Fs (one), 4 Fs (a cell across workgroups, finished by the second kernel); where Fs is 4, the shortest cell, 4 stands
for the first two."""
import ctypes as C

import numpy as np
import pytest

import survey_scene as scene
from pycusdr_amd import _lib
from pycusdr_amd.channelizer import UniformChannelizer, cell_floor, cell_mask, cell_power, design_taps

pytestmark = pytest.mark.gpu

FS = scene.FS
EPS = 2.0 ** -24
C_BOUND = 4                       # tests/test_gpu_channelizer_uniform.py: twice the worst measured constant of the uniform kernel's outputs


def ceiling(M, T):
    """tests/test_gpu_channelizer_uniform.py: the first-order constant of the uniform kernel's error bound."""
    return -(-T // M) + 3 * int(np.log2(M)) + 2


SHAPES = [(8, 3, 37), (16, 5, 17), (32, 32, 32), (64, 32, 513), (64, 48, 1025), (256, 128, 2049), (256, 256, 4096)]
PLAN_F = {(32, 32, 32): 112, (64, 48, 1025): 48, (256, 128, 2049): 8, (256, 256, 4096): 4}
MAX_IN = 1 << 17


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return (np.array_equal(bits(a.power), bits(b.power)) and np.array_equal(bits(a.floor), bits(b.floor))
            and np.array_equal(a.mask, b.mask))


def quantise(x, fmt):
    if fmt == 'cf32':
        return x.astype(np.complex64)
    full = 32767 if fmt == 'sc16' else 127
    q = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) * full), -full - 1, full)
    return q.astype(np.int16 if fmt == 'sc16' else np.int8)


def noise(rs, n, fmt='cf32'):
    return quantise(0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n)), fmt)


def taps_of(rs, T):
    return (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)


def cell_lengths(Fs):
    return sorted({max(4, Fs // 2), max(4, Fs), 4 * max(4, Fs)})


def far_cell(D, L):
    """A first cell near 2^40 / D."""
    return ((1 << 40) // D) // L


@pytest.mark.parametrize('M, D, T', SHAPES)
def test_power_table_is_the_definition_on_the_devices_outputs(M, D, T):
    rs = np.random.RandomState(M + D + T)
    h = taps_of(rs, T)
    uz = UniformChannelizer(FS, M, D, h, max_in=MAX_IN)
    F, _ = uz.info()
    Fs = uz.survey_info()[0]
    assert Fs & (Fs - 1) == 0 and F // 2 < Fs <= F and F == PLAN_F.get((M, D, T), F)
    lengths = cell_lengths(Fs)
    assert len(lengths) == (2 if Fs == 4 else 3) and lengths[-1] >= 4 * Fs
    for L in lengths:
        uz.set_survey(L)
        assert uz.survey_info()[:2] == (Fs, L)
        for first in (0, far_cell(D, L)):
            in_base, n = uz.needed_input_cells(first, 5)
            assert n <= MAX_IN
            x = noise(rs, n)
            y = uz.process(in_base, x, first * L, 5 * L)
            assert y.shape == (M, 5 * L)
            want = cell_power(y, L)
            assert want.min() > 0
            for ncells in (1, 2, 5):
                got = uz.survey(in_base, x, first, ncells)
                assert got.power.shape == (ncells, M) and got.power.dtype == np.float32
                assert np.array_equal(bits(got.power), bits(want[:ncells])), (L, first, ncells)
    uz.close()


@pytest.mark.parametrize('M, D, T', SHAPES)
def test_floor_and_mask_are_the_definitions_on_the_devices_table(M, D, T):
    rs = np.random.RandomState(M + D + T + 1)
    h = taps_of(rs, T)
    uz = UniformChannelizer(FS, M, D, h, bins=[1], max_in=MAX_IN)
    L = max(4, uz.survey_info()[0])
    uz.set_survey(L)
    in_base, n = uz.needed_input_cells(3, 3)
    # noise, and a tone between two bins that lifts a few of them far above the rest
    x = noise(rs, n).astype(np.complex128) + 0.2 * np.exp(2j * np.pi * (5.2 / M) * (in_base + np.arange(n)))
    x = x.astype(np.complex64)
    seen = set()
    for rank in (0, M // 4, M - 1):
        for thr in (1.0, 4.0):
            uz.set_survey(L, rank=rank, threshold=thr)
            assert uz.survey_info() == (uz.survey_info()[0], L, rank, thr)
            r = uz.survey(in_base, x, 3, 3)
            floor = cell_floor(r.power, rank)
            assert np.array_equal(bits(r.floor), bits(floor)), (rank, thr)
            mask = cell_mask(r.power, floor, thr)
            assert r.mask.shape == (3, -(-M // 32)) and r.mask.dtype == np.uint32
            assert np.array_equal(r.mask, mask), (rank, thr)
            assert np.array_equal(r.occupied(), r.power > (np.float32(thr) * floor)[:, None])
            seen.add(int(r.occupied().sum()))
    assert 0 in seen and 3 * (M - 1) in seen and len(seen) >= 3      # rank M - 1 sets nothing; rank 0 at threshold 1 all but the floor's bin
    uz.close()


@pytest.mark.parametrize('M, D, T, which', [(8, 3, 37, 0), (32, 32, 32, 2), (64, 48, 1025, 0), (64, 48, 1025, 2), (256, 128, 2049, 1),
                                            (256, 256, 4096, 1)])
def test_pure_function_of_position(M, D, T, which):
    """The same cells from one call, from single-cell calls, from a wider input window, from either output set, from device memory,
    with outputs written or not, and with one bin selected against all: identical bits in power, floor and mask."""
    import torch
    rs = np.random.RandomState(M + T + which)
    h = taps_of(rs, T)
    every = UniformChannelizer(FS, M, D, h, max_in=MAX_IN)
    one = UniformChannelizer(FS, M, D, h, bins=[M - 3], max_in=MAX_IN)
    L = cell_lengths(every.survey_info()[0])[min(which, len(cell_lengths(every.survey_info()[0])) - 1)]
    first, ncells = far_cell(D, L) + 1, 4
    every.set_survey(L, threshold=1.0)
    one.set_survey(L, threshold=1.0)
    in_base, n = every.needed_input_cells(first, ncells)
    lead = 7
    x = noise(rs, lead + n + 9)                              # positions in_base - lead .. in_base + n + 9
    core = x[lead:lead + n]
    whole = every.survey(in_base, core, first, ncells, buffer=0)
    assert 0 < whole.occupied().sum() < whole.occupied().size
    assert same(whole, every.survey(in_base - lead, x, first, ncells, buffer=1))                 # a wider window, the other set
    assert same(whole, one.survey(in_base, core, first, ncells))                                 # another selection
    res, out = one.survey(in_base - lead, x, first, ncells, write=True)                          # written
    assert same(whole, res)
    dev = torch.from_numpy(x).cuda()
    assert same(whole, every.survey(in_base, (dev.data_ptr() + 8 * lead, n), first, ncells))      # from device memory
    for s in range(ncells):
        b, c = every.needed_input_cells(first + s, 1)
        part = every.survey(b, x[b - in_base + lead:b - in_base + lead + c], first + s, 1, write=bool(s & 1), buffer=s & 1)
        part = part[0] if s & 1 else part
        assert part.first_cell == first + s
        assert np.array_equal(bits(part.power), bits(whole.power[s:s + 1])), s
        assert np.array_equal(bits(part.floor), bits(whole.floor[s:s + 1])) and np.array_equal(part.mask, whole.mask[s:s + 1]), s
    half = every.survey(in_base, core, first, 2)
    rest_base, rest_n = every.needed_input_cells(first + 2, 2)
    rest = every.survey(rest_base, x[rest_base - in_base + lead:rest_base - in_base + lead + rest_n], first + 2, 2)
    assert np.array_equal(bits(np.r_[half.power, rest.power]), bits(whole.power))
    every.close()
    one.close()


@pytest.mark.parametrize('M, D, T', [(16, 5, 17), (32, 32, 32), (64, 48, 1025), (256, 256, 4096)])
def test_writing_is_untouched(M, D, T):
    """write=True gives the bits of a plain process() of the span; a plain process() on a handle with a survey set those of one
    without; the outputs stand in the output set asked for."""
    rs = np.random.RandomState(M + T + 7)
    h = taps_of(rs, T)
    sel = [M - 1, 2, M // 2, 0, 5]
    plain = UniformChannelizer(FS, M, D, h, bins=sel, max_in=MAX_IN)
    uz = UniformChannelizer(FS, M, D, h, bins=sel, max_in=MAX_IN)
    for L in cell_lengths(uz.survey_info()[0]):
        uz.set_survey(L)
        first = far_cell(D, L)
        in_base, n = uz.needed_input_cells(first, 3)
        x = noise(rs, n)
        want = plain.process(in_base, x, first * L, 3 * L)
        res, out = uz.survey(in_base, x, first, 3, write=True, buffer=1)
        assert out.shape == want.shape == (len(sel), 3 * L) and np.array_equal(bits(out), bits(want)), L
        ptr, cnt = uz.device_output(1, 2)
        assert cnt == 3 * L and ptr % 16 == 0
        assert same(res, uz.survey(in_base, x, first, 3))
        # an odd span from an odd base through the plain call of the handle that has a survey set
        b, c = uz.needed_input(first * L + 3, 2 * L - 5)
        assert np.array_equal(bits(uz.process(b, x[b - in_base:b - in_base + c], first * L + 3, 2 * L - 5)), bits(want[:, 3:2 * L - 2])), L
    plain.close()
    uz.close()


@pytest.mark.parametrize('fmt, M, D, T', [('sc16', 64, 32, 513), ('sc8', 8, 3, 37)])
def test_integer_formats_equal_their_floats(fmt, M, D, T):
    """An sc16 / sc8 plan gives, bit for bit, the tables that a cf32 plan gives on raw.astype(float32) * scale."""
    rs = np.random.RandomState(17)
    h = taps_of(rs, T)
    scale = 2.0 ** -15 if fmt == 'sc16' else 2.0 ** -7
    a = UniformChannelizer(FS, M, D, h, sample_format=fmt, sample_scale=scale, max_in=MAX_IN)
    b = UniformChannelizer(FS, M, D, h, max_in=MAX_IN)
    for L in cell_lengths(a.survey_info()[0]):
        a.set_survey(L, threshold=1.5)
        b.set_survey(L, threshold=1.5)
        in_base, n = a.needed_input_cells(2, 3)
        raw = noise(rs, n, fmt)
        f = raw.astype(np.float32) * np.float32(scale)
        ra = a.survey(in_base, raw, 2, 3)
        rb = b.survey(in_base, (f[:, 0] + 1j * f[:, 1]).astype(np.complex64), 2, 3)
        assert same(ra, rb) and ra.power.min() > 0, L
    a.close()
    b.close()


WORST = {}


@pytest.mark.parametrize('M, D, T', SHAPES)
def test_device_within_the_derived_bound_of_the_host_back_end(M, D, T):
    """|P_dev - P_host| <= sum_m (2 |y_m| e_m + e_m^2) + (l + 2) 2^-24 P_host over the cell's frames, with
    e_m = sqrt(2) C_BOUND ceiling(M, T) 2^-24 S_m the modulus of the device's error in y_m (both components within
    C_BOUND ceiling 2^-24 S_m of the model, tests/test_gpu_channelizer_uniform.py), | |a|^2 - |b|^2 | <= 2 |b| |a - b| + |a - b|^2, and
    l + 2 roundings of relative 2^-24 on the way from the squares to the cell's sum (a product, the sum of the two, l levels), on
    either side; the host's rounding of y to complex64 is far inside e_m."""
    rs = np.random.RandomState(M + D + T + 3)
    h = taps_of(rs, T)
    dev = UniformChannelizer(FS, M, D, h, max_in=MAX_IN)
    host = UniformChannelizer(FS, M, D, h, backend='host', max_in=MAX_IN)
    worst = 0.0
    for L in cell_lengths(dev.survey_info()[0]):
        dev.set_survey(L)
        host.set_survey(L)
        for first in (0, far_cell(D, L)):
            in_base, n = dev.needed_input_cells(first, 2)
            x = noise(rs, n)
            pd, ph = dev.survey(in_base, x, first, 2), host.survey(in_base, x, first, 2)
            y, S = host.model(in_base, x, first * L, 2 * L)
            e = np.sqrt(2.0) * C_BOUND * ceiling(M, T) * EPS * S
            slack = (2 * np.abs(y) * e + e * e).reshape(M, 2, L).sum(axis=2).T + (int(np.log2(L)) + 2) * EPS * ph.power.astype(np.float64)
            assert slack.min() > 0
            ratio = float((np.abs(pd.power.astype(np.float64) - ph.power.astype(np.float64)) / slack).max())
            worst = max(worst, ratio)
    WORST[(M, D, T)] = worst
    print(f'M {M} D {D} T {T}: worst |P_dev - P_host| / bound = {worst:.4f}; so far {WORST}')
    dev.close()
    assert worst <= 1.0


def test_the_scene_on_the_device():
    dev = UniformChannelizer(FS, scene.M, scene.D, scene.TAPS, bins=[3, scene.M - 5], max_in=1 << 12)
    host = UniformChannelizer(FS, scene.M, scene.D, scene.TAPS, backend='host', max_in=1 << 12)
    for uz in (dev, host):
        uz.set_survey(scene.L, threshold=scene.THRESHOLD)
    in_base, n = dev.needed_input_cells(0, scene.NCELLS)
    x = scene.capture(n)
    rd, rh = dev.survey(in_base, x, 0, scene.NCELLS), host.survey(in_base, x, 0, scene.NCELLS)
    assert np.array_equal(rd.mask, rh.mask)
    occupied, judged = scene.expectation()
    assert np.array_equal(rd.occupied()[judged], occupied[judged])
    assert [(r['bin'], r['first_cell'], r['last_cell']) for r in rd.bursts()] == [(r['bin'], r['first_cell'], r['last_cell']) for r in rh.bursts()]
    dev.close()


def test_every_misuse_is_an_error_code():
    import torch
    lib = _lib.load()
    ARG, STATE, UNSUP, OK = _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED, _lib.MFB_OK
    M, D, T, L = 16, 4, 9, 8
    taps = np.linspace(0.1, 0.9, T).astype(np.float32)
    sel = np.array([3, 15], dtype=np.int32)
    words = np.array([1 << 60, 0], dtype=np.uint64)
    dev = torch.zeros(4096, dtype=torch.complex64, device='cuda')
    out = np.empty((2, 1024), np.complex64)
    power, floor, mask = np.empty((128, M), np.float32), np.empty(128, np.float32), np.empty((128, 1), np.uint32)
    ptr, cnt, ms = C.c_void_p(), C.c_int64(), C.c_float()

    def params(**kw):
        d = dict(in_base=0, out_base=0, device_input=dev.data_ptr(), in_count=4096, out_count=1000, input=2, buffer=0)
        d.update(kw)
        return _lib.ChannelizerParams(**d)

    def sbegin(h, write=0, **kw):
        return lib.mfb_channelizer_survey_begin(h, C.byref(params(**kw)), write)

    def send(h, o=None):
        return lib.mfb_channelizer_survey_end(h, o, power.ctypes.data, floor.ctypes.data, mask.ctypes.data)

    def good(h):
        """The handle still works: a survey with outputs, a survey without, a plain call."""
        assert sbegin(h, 1) == OK and send(h, out.ctypes.data) == OK
        assert sbegin(h, 0, out_base=L, out_count=2 * L) == OK and send(h) == OK
        assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK and lib.mfb_channelizer_end(h, out.ctypes.data) == OK

    # a survey belongs to the uniform plan: nothing of it on a direct or a rational handle
    plain = C.c_void_p()
    assert lib.mfb_channelizer_create(C.byref(plain), 0, 4, 64, 4096, 1024) == OK
    for rational in (False, True):
        if rational:
            assert lib.mfb_channelizer_set_plan_rational(plain, 3, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == OK
        else:
            assert lib.mfb_channelizer_set_plan(plain, D, taps.ctypes.data, T, words.ctypes.data, 2, 0, 1.0) == OK
        assert lib.mfb_channelizer_set_survey(plain, L, 4, 4.0) == STATE
        assert lib.mfb_channelizer_set_survey(plain, 0, 0, 1.0) == STATE
        assert lib.mfb_channelizer_survey_info(plain, None, None, None, None) == STATE
        assert sbegin(plain, out_count=1000 // (3 if rational else 1)) == STATE
        assert send(plain) == STATE
        assert lib.mfb_channelizer_begin(plain, C.byref(params(out_count=300))) == OK
        assert send(plain) == STATE                                          # a plain call in flight on a plain handle
        assert lib.mfb_channelizer_end(plain, None) == OK
    assert lib.mfb_channelizer_destroy(plain) == OK

    h = C.c_void_p()
    assert lib.mfb_channelizer_create_uniform(C.byref(h), 0, M, 4, 64, 4096, 1024) == OK
    # NULL handles; before a plan
    assert lib.mfb_channelizer_set_survey(None, L, 4, 4.0) == ARG and sbegin(None) == ARG and send(None) == ARG
    assert lib.mfb_channelizer_survey_info(None, None, None, None, None) == ARG
    assert lib.mfb_channelizer_set_survey(h, L, 4, 4.0) == STATE
    assert lib.mfb_channelizer_survey_info(h, None, None, None, None) == STATE
    assert sbegin(h) == STATE and send(h) == STATE
    assert lib.mfb_channelizer_set_plan_uniform(h, D, taps.ctypes.data, T, sel.ctypes.data, 2, 0, 1.0) == OK
    # no survey set
    a, b, r, t = C.c_int(), C.c_int(), C.c_int(), C.c_float()
    assert lib.mfb_channelizer_survey_info(h, C.byref(a), C.byref(b), C.byref(r), C.byref(t)) == OK and (a.value, b.value) == (0, 128)
    assert sbegin(h) == STATE and send(h) == STATE
    # set_survey: ARG
    for cell in (3, 12, 2, 1, -8, 1 << 17, 2048):                            # 2048: a power of two, longer than max_out
        assert lib.mfb_channelizer_set_survey(h, cell, 4, 4.0) == ARG, cell
    for rank in (-1, M):
        assert lib.mfb_channelizer_set_survey(h, L, rank, 4.0) == ARG
    for thr in (0.5, -4.0, float('nan'), float('inf')):
        assert lib.mfb_channelizer_set_survey(h, L, 4, thr) == ARG
    assert sbegin(h) == STATE                                                # every refusal left it unset
    assert lib.mfb_channelizer_set_survey(h, L, 4, 4.0) == OK
    assert lib.mfb_channelizer_survey_info(h, C.byref(a), C.byref(b), C.byref(r), C.byref(t)) == OK
    assert (a.value, b.value, r.value, t.value) == (L, 128, 4, 4.0)
    good(h)
    # survey_begin: ARG
    assert lib.mfb_channelizer_survey_begin(h, None, 0) == ARG
    for kw in (dict(out_base=4), dict(out_count=996), dict(out_base=4, out_count=996), dict(out_count=L + 1)):
        assert sbegin(h, **kw) == ARG, kw
        good(h)
    for kw in (dict(in_count=0), dict(out_count=0), dict(in_base=-1), dict(out_base=-L), dict(buffer=2), dict(input=3), dict(device_input=None),
               dict(device_input=dev.data_ptr() + 4), dict(in_count=4097), dict(out_count=1032), dict(in_base=8, out_base=0, out_count=L)):
        assert sbegin(h, **kw) == ARG, kw
    for kw in (dict(in_count=(1 << 24) + 1), dict(out_count=1 << 23), dict(in_base=1 << 62), dict(out_base=(1 << 62) // D)):
        assert sbegin(h, **kw) == UNSUP, kw
    assert sbegin(h, input=1) == STATE                                       # a pinned input never asked for
    good(h)
    # in flight
    assert sbegin(h) == OK
    assert sbegin(h, buffer=1) == STATE
    assert lib.mfb_channelizer_begin(h, C.byref(params(buffer=1))) == STATE
    assert lib.mfb_channelizer_set_survey(h, 2 * L, 4, 4.0) == STATE
    assert lib.mfb_channelizer_set_survey(h, 0, 0, 1.0) == STATE
    assert lib.mfb_channelizer_end(h, None) == STATE                         # a survey call ends with _survey_end
    assert lib.mfb_channelizer_end(h, out.ctypes.data) == STATE
    assert send(h, out.ctypes.data) == ARG                                   # nothing was written; the call stays in flight
    assert send(h) == OK
    assert send(h) == STATE
    assert lib.mfb_channelizer_device_output(h, 0, 0, C.byref(ptr), C.byref(cnt)) == STATE      # write_outputs = 0 left set 0 unwritten
    assert lib.mfb_channelizer_elapsed_ms(h, C.byref(ms)) == OK and ms.value > 0
    good(h)
    assert lib.mfb_channelizer_device_output(h, 0, 1, C.byref(ptr), C.byref(cnt)) == OK and cnt.value == 1000
    # a plain call ends with _end
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK
    assert send(h) == STATE
    assert lib.mfb_channelizer_end(h, None) == OK
    good(h)
    # every pointer of _survey_end may be NULL
    assert sbegin(h, 1) == OK and lib.mfb_channelizer_survey_end(h, None, None, None, None) == OK
    assert sbegin(h, 0) == OK and lib.mfb_channelizer_survey_end(h, None, None, floor.ctypes.data, None) == OK
    # a new plan drops the survey; turning it off does
    assert lib.mfb_channelizer_set_plan_uniform(h, D, taps.ctypes.data, T, sel.ctypes.data, 2, 0, 1.0) == OK
    assert sbegin(h) == STATE
    assert lib.mfb_channelizer_set_survey(h, L, 4, 4.0) == OK
    good(h)
    assert lib.mfb_channelizer_set_survey(h, 0, -1, 0.0) == OK               # off: rank and threshold do not matter
    assert sbegin(h) == STATE
    assert lib.mfb_channelizer_begin(h, C.byref(params())) == OK and lib.mfb_channelizer_end(h, out.ctypes.data) == OK
    assert lib.mfb_channelizer_destroy(h) == OK

    # the limits: M out_count <= 2^26, M out_count / L <= 2^22
    big = C.c_void_p()
    wide = torch.zeros(1 << 20, dtype=torch.complex64, device='cuda')
    t2 = np.ones(2, np.float32)
    zero = np.zeros(1, np.int32)
    assert lib.mfb_channelizer_create_uniform(C.byref(big), 0, 256, 1, 2, 1 << 20, 1 << 19) == OK
    assert lib.mfb_channelizer_set_plan_uniform(big, 2, t2.ctypes.data, 2, zero.ctypes.data, 1, 0, 1.0) == OK
    assert lib.mfb_channelizer_set_survey(big, 4, 64, 4.0) == OK

    def bparams(out_count):
        return _lib.ChannelizerParams(in_base=0, out_base=0, device_input=wide.data_ptr(), in_count=1 << 20, out_count=out_count, input=2,
                                      buffer=0)
    assert lib.mfb_channelizer_survey_begin(big, C.byref(bparams((1 << 18) + 4)), 0) == UNSUP        # 256 frames > 2^26
    assert lib.mfb_channelizer_survey_begin(big, C.byref(bparams(4 * ((1 << 14) + 1))), 0) == UNSUP  # 256 cells > 2^22
    assert lib.mfb_channelizer_survey_begin(big, C.byref(bparams(4 * (1 << 14))), 0) == OK           # the most cells of a call
    tab = np.empty(((1 << 14), 256), np.float32)
    assert lib.mfb_channelizer_survey_end(big, None, tab.ctypes.data, None, None) == OK
    assert np.all(tab == 0.0)
    assert lib.mfb_channelizer_destroy(big) == OK


def test_cycles_return_device_memory():
    import torch
    rs = np.random.RandomState(9)
    n = 1 << 14
    x = noise(rs, n, 'sc16')
    taps = design_taps(16)

    def cycle():
        uz = UniformChannelizer(FS, 64, 16, taps, bins=[1, 63], sample_format='sc16', sample_scale=2.0 ** -15, max_in=n, max_out=1 << 14)
        uz.set_survey(4)                                  # partials and table: max_out / 4 chunks and cells of 64 floats each
        uz.survey(0, x, 0, 64)
        uz.set_survey(256)
        uz.survey(0, x, 0, 3, write=True)
        uz.close()
    assert 50 * 2 * ((1 << 14) // 4) * 64 * 4 > (32 << 20)    # the survey's buffers alone would cross the bound
    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f'50 cycles: device free {free0 >> 20} -> {free1 >> 20} MiB')
    assert abs(free0 - free1) < (32 << 20), (free0, free1)
