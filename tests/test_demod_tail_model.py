"""tests/demod_tail_model.py (what tests/test_gpu_demod_tail.py holds k_envelope, code_rate_body and centres_body to) against what it
restates -- the oracle's find_centres, code_rate_and_phase and envelope -- and its case tables through the model alone: every case
reaches the branch it is named for.  No GPU."""
import numpy as np
import pytest

from oracle import mfbank_oracle as orc

import demod_tail_model as dm


@pytest.mark.parametrize('op', dm.CENTRES_OP)
@pytest.mark.parametrize('W', dm.CENTRES_W)
def test_centres_model_equals_the_oracle(W, op):
    """NaN-free small-integer signals, fractional rates and offsets, starts in front of sample 0 and behind the end."""
    rs = np.random.RandomState(100 * W + op)
    for lenSig in (6, 37, 300):
        for M in dm.CENTRES_M:
            for spSym, offset in ((2.0, 0.0), (2.5, 0.75), (3.3, 2.9), (7.01, 0.25), (float(lenSig) / 2, 1.5)):
                sig = dm.centres_signal(rs, 'random', M, lenSig)
                osym, ocen, omag = orc.find_centres(sig, spSym, offset, W, op)
                S = len(osym)
                assert S == int(lenSig / spSym)
                if S == 0:
                    continue
                sym, cen, mag, _ = dm.centres_model(sig, W, op, spSym, offset, S, S)
                assert np.array_equal(sym[:S], osym) and np.array_equal(cen[:S], ocen), (lenSig, M, spSym, offset)
                assert np.array_equal(mag[:S].view(np.uint32), omag.view(np.uint32))
                assert np.all(sym[S:].view(np.uint32) == dm.CANARY)


@pytest.mark.parametrize('family', ['e0', 'e60', 'em70', 'em80', 'mixed'])
def test_code_rate_model_equals_the_oracle(family):
    """The oracle takes an envelope: the one whose spectrum is P (bins 0 and n - 1 of a real signal's spectrum are real).  Unique
    maxima only -- float64 rounding of the round trip breaks exact ties -- which lead every other value by 2 (mixed: 18)."""
    rs = np.random.RandomState(dm.FAMILIES.index(family))
    n = 2053
    checked = 0
    for n_, off, ln in dm.code_rate_windows():
        if n_ != n or ln == 0:
            continue
        for name, pos in dm.peak_positions(ln).items():
            if name.startswith('tie') or off + pos[0] in (0, n - 1):
                continue
            P, winner = dm.code_rate_window(rs, family, n, off, ln, pos)
            P[0], P[n - 1] = P[0].real, P[n - 1].real
            env = np.fft.irfft(P.astype(np.complex128), 2 * (n - 1))
            ok, oarg, oval = orc.code_rate_and_phase(env, off, ln)
            k, re, im, val, ordered = dm.code_rate_model(P, off, ln)
            assert k == ok == winner and ordered == ln, (off, ln, name)
            assert abs(np.arctan2(float(im), float(re)) - oarg) < 1e-9
            exact = dm._abs2_key(P[k])[1] / (1 << (2 * dm._EXP0))
            assert abs(exact - oval) <= 1e-9 * oval
            checked += 1
    assert checked >= 20


def test_envelope_model_equals_the_oracle():
    rs = np.random.RandomState(5)
    for M in dm.ENVELOPE_M:
        xc = dm.envelope_input(rs, 1, M, 33)[0]
        offs = dm.envelope_offsets(M)
        assert offs == list(range((M + 1) // 2)) and all(2 * o < M for o in offs) and 2 * (offs[-1] + 1) >= M
        for off in offs:
            assert np.array_equal(dm.envelope_model(xc, off).astype(np.float64), orc.envelope(xc, off))
    assert dm.ENVELOPE_TWO_ITERATIONS > 1024 * 256          # k_envelope's grid: 1024 workgroups of 256 threads


@pytest.mark.parametrize('family', dm.FAMILIES)
def test_code_rate_cases_reach_their_branches(family):
    cases = dm.code_rate_cases(family)
    assert {(n, off, ln) for n, off, ln, *_ in cases} == set(dm.code_rate_windows())
    seen, fallback = set(), 0
    for n, off, ln, name, P, winners in cases:
        assert P.dtype == np.complex64 and P.shape[1] == n
        seen.add((n, len(P)))
        for b, nm in enumerate(name.split('+')):
            k, re, im, val, ordered = dm.code_rate_model(P[b], off, ln)
            assert k == winners[b], (n, off, ln, nm)
            fallback += (k == 0 and off == 0 and ln > 0)
            if ln == 0:
                assert (k, val) == (0, -1.0)
                continue
            key = dm._abs2_key(P[b][k])
            # larger values just outside the window
            for g in (off - 1, off + ln):
                if 0 <= g < n and key is not None and not key[0]:
                    assert dm._abs2_key(P[b][g]) > key
            pos = dm.peak_positions(ln).get(nm, ())
            if nm.startswith('tie') and family not in ('one_inf', 'two_inf'):
                p, q = pos
                assert k == off + p and q > p and dm._abs2_key(P[b][off + q]) == key and P[b][off + q] != P[b][off + p]
                assert {'tie_adjacent': q - p == 1, 'tie_same_thread': q - p == 1024, 'tie_1023': q - p == 1023, 'tie_ends': (p, q) == (0, ln - 1),
                        'tie_first_last_wave': p < 64 and 960 <= q < 1024}[nm]
                # nothing else reaches the maximum
                assert sum(dm._abs2_key(z) == key for z in P[b][off:off + ln]) == 2
            if family == 'e60':
                # every unscaled fp32 square around the peak overflows: without the exact scaling they would all tie at +inf
                with np.errstate(over='ignore'):
                    sq = (P[b][off:off + ln].real.astype(np.float32) ** 2 + P[b][off:off + ln].imag.astype(np.float32) ** 2)
                assert np.isinf(val) and (ln < 3 or np.isinf(sq).sum() > ln // 2)
            elif family in ('em70', 'em80'):
                # the unscaled fp32 squares: below the normal range for the window's small values (em70), for every value (em80)
                small = [z for z in P[b][off:off + ln] if 0 < dm._abs2_key(z)[1] / (1 << (2 * dm._EXP0)) < 2.0 ** -126]
                assert key[1] > 0 and (ln < 1023 or small) and (family == 'em70' or len(small) == np.count_nonzero(P[b][off:off + ln]))
            elif family == 'zero':
                assert ordered == ln and k == off and val == 0 and not P[b][off:off + ln].any()
            elif family == 'all_nan':
                assert ordered == 0 and k == off and val is None
            elif family == 'nan_scattered':
                assert (0 < ordered < ln or ln <= 5) and val is not None
                assert ln < 6 or np.isnan(P[b][off].real) or np.isnan(P[b][off].imag) or k == off
            elif family == 'one_inf':
                assert np.isinf(val) and sum(dm._abs2_key(z) == (1, 0) for z in P[b][off:off + ln]) == 1
            elif family == 'two_inf':
                infs = [x for x in range(off, off + ln) if dm._abs2_key(P[b][x]) == (1, 0)]
                assert np.isinf(val) and k == infs[0] and len(infs) == min(2, ln)
                assert ln <= 2048 or infs[1] - infs[0] == 1024
            elif family == 'neg_zero':
                win = P[b][off:off + ln]
                assert (ln < 4 or np.signbit(win.real).any()) and (nm != 'none' or (np.signbit(win.real).all() and np.signbit(win.imag).all() and k == off))
    assert seen >= {(1, 1), (1, 3), (7, 1), (7, 3), (2053, 1), (2053, 3), (4101, 1), (4101, 3)}
    if family in ('e0', 'e60', 'em70', 'em80'):
        assert fallback                        # offset 0 with the maximum in bin 0: k* = 0, the spSym = 10 fall-back
        names = {nm for *_, name, _, _ in cases for nm in name.split('+')}
        assert names >= {'first', 'last', 'middle', 'tie_adjacent', 'tie_same_thread', 'tie_1023', 'tie_first_last_wave', 'tie_ends'}


ALL_CENTRES_TAGS = {'canary', 'cut_by_end', 'nan_and_zero', 'nan_only', 'nan_skipped', 'neg_start', 'neg_start_frac', 'sentinel',
                    'start_at_len', 'start_last', 'tie_filters', 'tie_positions', 'zero_window'}


@pytest.mark.parametrize('lenSig', dm.CENTRES_LEN)
def test_centres_cases_reach_their_branches(lenSig):
    reached = {op: set() for op in dm.CENTRES_OP}
    for op in dm.CENTRES_OP:
        cases = dm.centres_cases(lenSig, op)
        assert {(c['sig'].shape[0], c['W']) for c in cases} == {(M, W) for M in dm.CENTRES_M for W in dm.CENTRES_W}
        assert {c['nthreads'] for c in cases} == {1, 256, 257}
        assert {np.sign(c['capacity'] - c['nthreads']) for c in cases} == {-1, 0, 1}
        assert {c['pattern'] for c in cases} == set(dm.SIG_PATTERNS)
        for c in cases:
            sym, cen, mag, tags = dm.centres_model(c['sig'], c['W'], c['op'], c['spSym'], c['offset'], c['capacity'], c['nthreads'])
            assert c['tags'] <= tags, (c['name'], c['tags'] - tags)
            assert len(sym) == (c['nthreads'] + 255) // 256 * 256
            assert np.all(sym[c['capacity']:].view(np.uint32) == dm.CANARY) and np.all(mag[c['capacity']:].view(np.uint32) == dm.CANARY)
            assert not np.any(sym[:c['capacity']].view(np.uint32) == dm.CANARY)
            live = (sym != dm.INT32_MIN) & (sym.view(np.uint32) != dm.CANARY)
            if live.any():
                if c['pattern'] == 'zero':
                    assert 'zero_window' in tags and np.all(sym[live] == -1)
                if c['pattern'] == 'nan_all':
                    assert 'nan_only' in tags and np.all(sym[live] == -1)
                if c['pattern'] == 'constant':
                    assert np.all(sym[live] == 0)
                if c['pattern'] == 'negative' and op and lenSig > 1:
                    assert 'negative_maximum' in tags
            reached[op] |= tags
    if lenSig >= 37:
        for op in dm.CENTRES_OP:
            assert reached[op] >= ALL_CENTRES_TAGS | ({'negative_maximum'} if op else set()), (op, ALL_CENTRES_TAGS - reached[op])


def test_centres_overflow_case_passes_int32():
    c = dm.OVERFLOW_CASE
    sig = dm.centres_signal(np.random.RandomState(1), 'random', c['M'], c['lenSig'])
    sym, cen, mag, tags = dm.centres_model(sig, c['W'], 0, c['spSym'], c['offset'], c['capacity'], c['nthreads'])
    assert 'beyond_int32' in tags and 71 * c['spSym'] < 2 ** 31 <= 72 * c['spSym']
    assert sym[0] >= 0 and np.all(sym[1:] == dm.INT32_MIN) and np.all(cen[1:] == dm.INT32_MIN) and not mag[1:].any()


def test_seams_check_their_arguments_before_touching_a_device():
    """The three seams are additive (found by symbol: the ABI version stays) and refuse bad arguments without a GPU."""
    from pycusdr_amd import _lib
    lib = _lib.load()
    assert lib.mfb_abi_version() == 9
    z = np.zeros(64, np.complex64)
    p = z.ctypes.data
    assert lib.mfb_debug_envelope(0, None, 1, 1, 1, 0, p) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_envelope(0, p, 1, 4, 4, 2, p) == _lib.MFB_ERR_ARG               # 2 * off >= M
    assert lib.mfb_debug_envelope(0, p, 1, 1, 0, 0, p) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_envelope(0, p, 1, 64, 1 << 21, 0, p) == _lib.MFB_ERR_UNSUPPORTED
    assert lib.mfb_debug_code_rate(0, p, 1, 8, 4, 5, 0, 0, p, p, p, p, p) == _lib.MFB_ERR_ARG     # offset + len > n
    assert lib.mfb_debug_code_rate(0, p, 1, 8, -1, 2, 0, 0, p, p, p, p, p) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_code_rate(0, p, 1, 8, 0, 2, 0, 0, p, p, None, p, p) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_centres(0, p, 1, 8, 3, 0, 1.5, 0.0, 4, 4, p, p, p) == _lib.MFB_ERR_ARG   # spSym < 2
    assert lib.mfb_debug_centres(0, p, 1, 8, 3, 3, 2.0, 0.0, 4, 4, p, p, p) == _lib.MFB_ERR_ARG   # op
    assert lib.mfb_debug_centres(0, p, 1, 8, 3, 0, 2.0, 0.0, 4, (1 << 20) + 1, p, p, p) == _lib.MFB_ERR_UNSUPPORTED
