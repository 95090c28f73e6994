"""The three kernels between the matched filters and the bit stream -- k_envelope (and its fused twin in k_seg's STORE mode),
k_code_rate / k_code_rate_block, k_centres -- on INJECTED inputs, through the seams mfb_debug_envelope, mfb_debug_code_rate and
mfb_debug_centres, against tests/demod_tail_model.py: the smallest shapes at which each branch of the kernels exists, exact inputs
(integers times a power of two), results compared bit for bit.  The case tables are the model's; tests/test_demod_tail_model.py
shows on the host that every case reaches the branch it is named for."""
import numpy as np
import pytest

from oracle import mfbank_oracle as orc
from pycusdr_amd import mfbank
from pycusdr_amd.mfbank import MFBank

import demod_tail_model as dm

pytestmark = pytest.mark.gpu
U32 = np.uint32


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


# ------------------------------------------------------------------------------------------------------------------------------
# code rate
# ------------------------------------------------------------------------------------------------------------------------------
ARG_BOUND = 1e-4           # the suite's bound on arg P[k*] (test_demod_stage_matches_oracle)
SPSYM_MIN = 4


def _same_f(a, b):
    """Equal floats, NaN equal to NaN."""
    return bool(a == b or (a != a and b != b))


@pytest.mark.parametrize('family', dm.FAMILIES)
def test_code_rate_family(family):
    """Every window geometry of the table x every position of the maximum, in batches of 3 and 1: k* exact, |P[k*]|^2 bit for bit where
    the family defines it, the argument against float64 arctan2 of the same components, k_code_rate and k_code_rate_block equal bit
    for bit, and the block form's scalars equal to the host arithmetic (DB:733-752, 994-999)."""
    worst, fallbacks, windows = 0.0, 0, 0
    for n, off, ln, name, P, winners in dm.code_rate_cases(family):
        cap = n // 8                     # binds whenever spSym < 8
        r = mfbank.debug_code_rate(P, off, ln, SPSYM_MIN, cap)
        where = (family, n, off, ln, name)
        assert np.array_equal(_bits(r['triples']), _bits(r['block_triples'])), where
        for b in range(len(P)):
            k, re, im, val, _ = dm.code_rate_model(P[b], off, ln)
            gk, garg, gval = r['triples'][b]
            assert float(gk) == k == winners[b], (where, b, gk, k)
            if np.isnan(re) or np.isnan(im):
                assert np.isnan(garg) and (np.isnan(gval) if ln else _bits(gval) == _bits(np.float32(-1.0))), (where, b)
            else:
                err = abs(float(garg) - float(np.arctan2(np.float64(im), np.float64(re))))
                worst = max(worst, err)
                assert err < ARG_BOUND, (where, b, f'arg error {err:.3e}, the largest so far {worst:.3e}')
                if ln == 0:
                    assert _bits(gval) == _bits(np.float32(-1.0)), (where, b)
                elif family in dm.VAL_BITWISE:
                    assert _bits(gval) == _bits(val), (where, b, gval, val)
                elif family == 'mixed':
                    # fma(x, x, fl(y * y)): two roundings of 2^-24 each, relative to a sum of non-negative terms
                    exact = float(re) ** 2 + float(im) ** 2
                    assert abs(float(gval) - exact) <= 2.0 ** -23 * exact, (where, b)
            # the block form's scalars: the host's float64 arithmetic on the device's own fp32 triple, then the clamp and the count
            spSym, codeOffset = orc.code_rate_host(gk, garg, n)
            assert r['spSym'][b] == spSym and _same_f(r['codeOffset'][b], codeOffset), (where, b)
            assert r['rate_fallback'][b] == (k == 0) and (k != 0 or spSym == 10.0), (where, b)
            sp = max(spSym, float(SPSYM_MIN))
            assert _bits(r['spSymF'][b]) == _bits(np.float32(sp)), (where, b)
            assert _same_f(r['offsetF'][b], np.float32(codeOffset)), (where, b)
            assert r['count'][b] == min(int(n / sp), cap), (where, b)
            fallbacks += (k == 0 and off == 0 and ln > 0)
            windows += 1
    print(f'code rate [{family}]: {windows} windows, largest |arg - arctan2| = {worst:.3e}')
    assert windows >= 4 * len(dm.code_rate_windows())         # every geometry in a batch of 3 and in a batch of 1
    if family in ('e0', 'e60', 'em70', 'em80'):
        assert fallbacks                   # offset 0 and the maximum in bin 0: k* = 0 through k_code_rate_block


def test_code_rate_seam_refuses_what_demodulate_refuses():
    P = np.ones((2, 7), np.complex64)
    for off, ln in ((-1, 2), (0, -1), (7, 1), (3, 5), (8, 0)):
        with pytest.raises(ValueError):
            mfbank.debug_code_rate(P, off, ln)
    assert mfbank.debug_code_rate(P, 7, 0)['triples'][1, 2] == -1.0
    with pytest.raises(TypeError):
        mfbank.debug_code_rate(P.astype(np.complex128), 0, 1)


@pytest.fixture(scope='module')
def bank10():
    """A handle at log2N = 10 holding a block: the real call's window arguments."""
    rs = np.random.RandomState(3)
    N, M = 1 << 10, 4
    bank = MFBank(10, 2, M)
    bank.set_filters(_short_masks(rs, M, N, 16))
    bank.set_shifts([0, 1])
    bank.upload((rs.standard_normal(N) + 1j * rs.standard_normal(N)).astype(np.complex64))
    yield bank
    bank.close()


def _short_masks(rs, M, N, T):
    h = np.zeros((M, N), np.complex128)
    h[:, :T] = rs.standard_normal((M, T)) + 1j * rs.standard_normal((M, T))
    return np.fft.fft(h, axis=1).astype(np.complex64)


@pytest.mark.parametrize('k_off', [0, 1, 511, 1024])
def test_demodulate_with_an_empty_window(bank10, k_off):
    """len == 0 -> {0, arg P[0], -1}; P[0] is the sum of the envelope, a sum of squares: real and positive."""
    k, arg, val = bank10.demodulate(3, k_off, 0)
    assert (float(k), float(arg), float(val)) == (0.0, 0.0, -1.0)


def test_demodulate_window_bounds(bank10):
    N = bank10.N
    k, _, val = bank10.demodulate(3, N - 5, 5)
    assert N - 5 <= k < N and val > 0
    k, _, val = bank10.demodulate(3, 0, N)
    assert 0 <= k < N and val > 0
    for off, ln in ((N - 5, 6), (0, N + 1), (N + 1, 0), (-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            bank10.demodulate(3, off, ln)


# ------------------------------------------------------------------------------------------------------------------------------
# centres
# ------------------------------------------------------------------------------------------------------------------------------
def _centres_equal(c, got, where):
    sym, cen, mag, _ = dm.centres_model(c['sig'], c['W'], c['op'], c['spSym'], c['offset'], c['capacity'], c['nthreads'])
    assert len(got[0]) == len(sym) == (c['nthreads'] + 255) // 256 * 256
    assert np.array_equal(got[0], sym), (where, np.flatnonzero(got[0] != sym)[:5])
    assert np.array_equal(got[1], cen), (where, np.flatnonzero(got[1] != cen)[:5])
    assert np.array_equal(_bits(got[2]), _bits(mag)), (where, np.flatnonzero(_bits(got[2]) != _bits(mag))[:5])


@pytest.mark.parametrize('op', dm.CENTRES_OP)
@pytest.mark.parametrize('lenSig', dm.CENTRES_LEN)
def test_centres_geometry(lenSig, op):
    """M x W x {dense, fractional, sparse, single, at_last, at_len} x the signal patterns: symbol, centre and magnitude of every entry,
    the sentinels behind the end, the canary from `capacity` on."""
    for c in dm.centres_cases(lenSig, op):
        got = mfbank.debug_centres(c['sig'], c['W'], c['op'], c['spSym'], c['offset'], c['capacity'], c['nthreads'])
        _centres_equal(c, got, c['name'])


def test_centres_conversion_overflow():
    """x * spSym passes 2^31 from x = 72 on: every symbol behind the first is past the end -- decided in float, before any conversion."""
    o = dm.OVERFLOW_CASE
    for op in dm.CENTRES_OP:
        c = dict(o, op=op, sig=dm.centres_signal(np.random.RandomState(op), 'random', o['M'], o['lenSig']))
        got = mfbank.debug_centres(c['sig'], c['W'], op, c['spSym'], c['offset'], c['capacity'], c['nthreads'])
        _centres_equal(c, got, ('overflow', op))
        assert got[0][0] >= 0 and np.all(got[0][1:] == dm.INT32_MIN) and np.all(got[1][1:] == dm.INT32_MIN) and not got[2][1:].any()


def test_centres_seam_refuses_bad_arguments():
    sig = np.ones((2, 8), np.complex64)
    for kw in (dict(W=0), dict(op=3), dict(spSym=1.5), dict(spSym=float('nan')), dict(offset=-1.0), dict(offset=float('nan')),
               dict(capacity=-1), dict(nthreads=0)):
        a = dict(W=3, op=0, spSym=2.0, offset=0.0, capacity=4, nthreads=4)
        a.update(kw)
        with pytest.raises(ValueError):
            mfbank.debug_centres(sig, **a)


# ------------------------------------------------------------------------------------------------------------------------------
# envelope
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', dm.ENVELOPE_N)
def test_envelope_seam(N):
    rs = np.random.RandomState(N)
    for M in dm.ENVELOPE_M:
        for nb in dm.ENVELOPE_NB:
            xc = dm.envelope_input(rs, nb, M, N)
            for off in dm.envelope_offsets(M):
                env = mfbank.debug_envelope(xc, off)
                assert env.shape == (nb, N)
                for b in range(nb):
                    assert np.array_equal(_bits(env[b]), _bits(dm.envelope_model(xc[b], off))), (N, M, nb, off, b)


def test_envelope_grid_stride_second_iteration():
    """N = 1024 * 256 + 3: three threads take a second element."""
    N = dm.ENVELOPE_TWO_ITERATIONS
    xc = dm.envelope_input(np.random.RandomState(9), 1, 1, N)
    env = mfbank.debug_envelope(xc[0], 0)
    want = (xc[0, 0].real.astype(np.int64) ** 2 + xc[0, 0].imag.astype(np.int64) ** 2).astype(np.float32)
    assert np.array_equal(_bits(want[-5:]), _bits(dm.envelope_model(xc[0, :, -5:], 0)))
    assert np.array_equal(_bits(env), _bits(want)), np.flatnonzero(env != want)[:5]


def test_envelope_seam_and_create_refuse_an_offset_that_leaves_no_filter():
    xc = np.ones((5, 8), np.complex64)
    for M, off in ((5, 3), (4, 2), (1, 1), (5, -1)):
        with pytest.raises(ValueError):
            mfbank.debug_envelope(xc[:M], off)
        with pytest.raises(ValueError):
            MFBank(12, 2, M, code_search_mask_offset=off)


@pytest.mark.parametrize('path,M', [('segment', 4), ('segment', 5), ('segment', 20), ('twopass', 4)])
def test_envelope_of_a_handle_with_a_mask_offset(path, M):
    """code_search_mask_offset > 0 through real handles: the segment path sums the envelope inside k_seg for M <= 16 and launches
    k_envelope above, the two-pass path launches k_envelope.  Either way the envelope equals k_envelope's on the handle's own
    matched-filter outputs BIT FOR BIT (the fused form's 'same fp32 order'; cs_off reaches the launch), and the oracle's to 1e-6
    of its peak."""
    log2N, N = 12, 1 << 12
    rs = np.random.RandomState(10 * M + len(path))
    masks = _short_masks(rs, M, N, 16)
    x = (rs.standard_normal(N) + 1j * rs.standard_normal(N)).astype(np.complex64)
    for off in ((0, 1, 2) if M == 5 else (0, 1)):
        bank = MFBank(log2N, 2, M, code_search_mask_offset=off)
        try:
            bank.set_filters(masks)
            bank.set_shifts([0, 1])
            bank.set_search_path(path)
            assert bank.get_search_path()['path'] == path
            bank.upload(x)
            bank.demodulate(5, 10, 100)
            xc, env = bank.get_xcorr(), bank.get_envelope()
        finally:
            bank.close()
        assert np.array_equal(_bits(env), _bits(mfbank.debug_envelope(xc, off))), (path, M, off)
        ref = orc.envelope(xc, off)
        assert np.abs(env - ref).max() < 1e-6 * ref.max(), (path, M, off)
        if off:
            assert np.abs(env - orc.envelope(xc, 0)).max() > 1e-3 * ref.max()          # the offset matters for this bank
