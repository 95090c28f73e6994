"""The three kernels between the matched filters and the bit stream (csrc/small_kernels.hpp: k_envelope, code_rate_body,
centres_body) restated as scalar Python loops, and the case tables that tests/test_demod_tail_model.py (host) and
tests/test_gpu_demod_tail.py (device, through the mfb_debug_envelope / _code_rate / _centres seams) share.

The inputs are chosen so that the models are EXACT without emulating a fused multiply-add: components are j * 2^e with integer
|j| <= 2047, so every square and every sum of two squares has at most 23 significant bits -- exact in fp32 and in integer
arithmetic alike.  The models are plain integer arithmetic on the bit patterns of the fp32 inputs.

  envelope   sumXCorrBuffMasks, CU:191-205: sum over the filters off <= m < M - off, ascending.
  code rate  findCodeRateAndPhase, CU:236-320, with the promises of code_rate_body's header: the maximum of |P[k]|^2 over the
             window's ordered values (no NaN component), the lowest k on ties, `offset` without an ordered value, and
             {0, arg P[0], -1} for an empty window.
  centres    findCentres, CU:78-146, line by line; symbols whose window starts at or behind the end get the sentinel INT32_MIN (the
             reference leaves them untouched), entries from `capacity` on are not written at all (CANARY stays).
"""
import functools
import math

import numpy as np

f32 = np.float32
INT32_MIN = -(1 << 31)
CANARY = 0x5a5a5a5a
CANARY_F32 = np.array([CANARY], np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------------------------------------------------------------------
# envelope
# ------------------------------------------------------------------------------------------------------------------------------
def envelope_model(xc, off):
    """xc complex64 [M][N] of small integers -> float32 [N]; the sums stay below 2^24 (asserted), so they are exact."""
    M, N = xc.shape
    re, im = xc.real.astype(np.int64).tolist(), xc.imag.astype(np.int64).tolist()
    out = [0] * N
    for m in range(off, M - off):
        rm, jm = re[m], im[m]
        for x in range(N):
            out[x] += rm[x] * rm[x] + jm[x] * jm[x]
    assert max(out) < 1 << 24
    return np.array(out, np.float32)


def envelope_input(rs, nb, M, N):
    """Integer components |j| <= 100: 17 filters * 2 * 100^2 < 2^24."""
    return (rs.randint(-100, 101, (nb, M, N)) + 1j * rs.randint(-100, 101, (nb, M, N))).astype(np.complex64)


ENVELOPE_N = (1, 255, 257, 4099)
ENVELOPE_M = (1, 2, 5, 17)
ENVELOPE_NB = (1, 3)
ENVELOPE_TWO_ITERATIONS = 1024 * 256 + 3          # the grid of 1024 workgroups x 256 threads strides once


def envelope_offsets(M):
    return [off for off in range(M) if 2 * off < M]


# ------------------------------------------------------------------------------------------------------------------------------
# code rate
# ------------------------------------------------------------------------------------------------------------------------------
_EXP0 = 149 + 24        # every finite fp32 is an integer multiple of 2^-149


def _exact_int(v):
    """A finite fp32 value as an integer multiple of 2^-_EXP0."""
    m, e = math.frexp(float(v))
    j = int(m * (1 << 24))
    assert j / (1 << 24) == m
    return j << (e - 24 + _EXP0)


def _abs2_key(z):
    """|z|^2 as something ordered: None for an unordered value (a NaN component), (1, 0) for +inf, (0, exact integer) else."""
    x, y = float(z.real), float(z.imag)
    if math.isnan(x) or math.isnan(y):
        return None
    if math.isinf(x) or math.isinf(y):
        return (1, 0)
    a, b = _exact_int(x), _exact_int(y)
    return (0, a * a + b * b)


def _key_f32(key):
    """The fp32 value of an exact |z|^2 (+inf beyond the range).  Python divides integers with one correct rounding, to float64; the
    values this is used for have at most 23 significant bits, so the second step, to fp32, rounds nothing but overflows."""
    with np.errstate(over='ignore'):
        return f32(np.inf) if key[0] else f32(key[1] / (1 << (2 * _EXP0)))


def code_rate_model(P, offset, length):
    """-> (k, re, im, val, ordered): k the winner, (re, im) the fp32 components of P[k] (the argument is left to the caller:
    atan2 is not exact), val the fp32 value of |P[k]|^2 (None where P[k] holds a NaN: any NaN), ordered = number of ordered values."""
    if length == 0:
        return 0, f32(P[0].real), f32(P[0].imag), f32(-1.0), 0
    best, k, ordered = None, offset, 0
    for x in range(offset, offset + length):
        key = _abs2_key(P[x])
        if key is None:
            continue
        ordered += 1
        if best is None or key > best:        # strict: the lowest k keeps a tie
            best, k = key, x
    key = _abs2_key(P[k])
    return k, f32(P[k].real), f32(P[k].imag), (None if key is None else _key_f32(key)), ordered


CODE_RATE_N = (1, 7, 2053, 4101)
CODE_RATE_LEN = (0, 1, 2, 1023, 1024, 1025, 2049, 3000)
PEAK, PEAK2 = (1500, 1400), (1400, -1500)       # the same |.|^2 = 4 210 000 with different arguments; the background stays <= 2 000 000
GUARD = (2047, 2047)                            # just outside the window: larger than the peak, and never to be chosen
BACKGROUND = 1000


def code_rate_windows():
    """Every (n, offset, len) of the issue's table that fits: len x offset in {0, 1, n - len}, offset + len <= n."""
    out = []
    for n in CODE_RATE_N:
        for ln in CODE_RATE_LEN:
            for off in sorted({0, 1, n - ln}):
                if 0 <= off and off + ln <= n:
                    out.append((n, off, ln))
    return out


def peak_positions(ln):
    """name -> window-relative positions of the (equal) maxima, the winner first.  A block of 1024 threads: element x goes to
    thread x % 1024, iteration x // 1024."""
    pos = {}
    if ln >= 1:
        pos['first'] = (0,)
        pos['last'] = (ln - 1,)
        pos['middle'] = (ln // 2,)
    if ln >= 2:
        pos['tie_adjacent'] = (ln // 3, ln // 3 + 1)
        pos['tie_ends'] = (0, ln - 1)
    if ln > 1023:
        p = (ln - 1023) // 2
        pos['tie_1023'] = (p, p + 1023)                 # thread t in iteration 0 against thread t - 1 in iteration 1
    if ln > 1024:
        p = (ln - 1024) // 2
        pos['tie_same_thread'] = (p, p + 1024)          # the thread's own strided loop: next iteration
    if ln > 1000:
        pos['tie_first_last_wave'] = (5, 1000)          # threads 5 (wave 0) and 1000 (wave 15): the last level of the LDS tree
    return pos


FAMILIES = ('e0', 'e60', 'em70', 'em80', 'mixed', 'zero', 'all_nan', 'nan_scattered', 'one_inf', 'two_inf', 'neg_zero')
FAMILY_EXP = {'e60': 60, 'em70': -70, 'em80': -80}
# families whose out[2] is defined bit for bit (em70, em80: the squares of the small values, at -80 of all values, are denormal, and
# whether those flush is not part of the contract; mixed: rounded)
VAL_BITWISE = ('e0', 'e60', 'zero', 'nan_scattered', 'one_inf', 'two_inf', 'neg_zero')


def _c(re, im, e=0):
    return complex(math.ldexp(re, e), math.ldexp(im, e))


def code_rate_window(rs, family, n, offset, ln, positions):
    """One spectrum complex64 [n] of `family` with equal maxima at the window-relative `positions` (lowest first) and larger values
    just outside the window.  -> (P, winner): the k the case is named for."""
    e = FAMILY_EXP.get(family, 0)
    re, im = rs.randint(-BACKGROUND, BACKGROUND + 1, n).tolist(), rs.randint(-BACKGROUND, BACKGROUND + 1, n).tolist()
    P = np.zeros(n, np.complex128)
    if family == 'mixed':
        # every background |P|^2 <= 2 * (1000 * 2^10)^2 = 2^21 * 10^6; the peak's is (1500 * 2^12)^2 = 2.25 * 2^24 * 10^6 and more: a lead
        # of 18, so rounding cannot change the winner; no ties in this family
        ex = rs.randint(-20, 11, (2, n)).tolist()
        for x in range(n):
            P[x] = complex(math.ldexp(re[x], ex[0][x]), math.ldexp(im[x], ex[1][x]))
    elif family == 'zero':
        P[:] = 0.0
    elif family == 'all_nan':
        P[:] = complex(np.nan, np.nan)
    elif family == 'neg_zero':
        P[:] = complex(-0.0, -0.0)
        if positions:                           # (without a planted peak: -0.0 and nothing else)
            for x in range(0, n, 3):
                P[x] = complex(-0.0, im[x] if x % 2 else 0.0)
    else:
        for x in range(n):
            P[x] = _c(re[x], im[x], e)
    winner = offset
    if family not in ('zero', 'all_nan') and positions:
        winner = offset + positions[0]
        for i, p in enumerate(positions):
            P[offset + p] = complex(math.ldexp(1500, 12), math.ldexp(3, -5)) if family == 'mixed' else _c(*(PEAK2 if i else PEAK), e)
    if family == 'nan_scattered':
        # NaN in the real part, the imaginary part or both, never on a planted peak; the window's first element among them
        peaks = {offset + p for p in positions}
        for i, x in enumerate(range(offset, offset + ln, 5)):
            if x not in peaks:
                P[x] = (complex(np.nan, 3.0), complex(-2.0, np.nan), complex(np.nan, np.nan))[i % 3]
    if family in ('one_inf', 'two_inf') and ln > 0:
        # +inf BEHIND the finite peak where there is room: it wins although the finite peak comes first
        if family == 'one_inf':
            spots = [ln - 1]
        else:
            spots = [ln // 2, ln // 2 + 1024] if ln > ln // 2 + 1024 else sorted({max(ln - 2, 0), ln - 1})
        for i, p in enumerate(spots):
            P[offset + p] = complex(3.0, -np.inf) if i else complex(np.inf, -7.0)
        winner = offset + spots[0]
    for g in (offset - 1, offset + ln):
        if 0 <= g < n:
            P[g] = complex(math.ldexp(2047, 14), 0.0) if family == 'mixed' else _c(*GUARD, e)
    if ln == 0:
        winner = 0
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return P.astype(np.complex64), winner


@functools.lru_cache(maxsize=None)
def code_rate_cases(family, seed=0):
    """The family's cases: (n, offset, len, name, P complex64 [nb][n], winners [nb]).  The peak positions of one window geometry
    are spread over the windows of batches of 3 (the last one filled up from the front); one more batch of 1 repeats the first
    position on another background: both batch sizes run at every geometry."""
    rs = np.random.RandomState(seed + 1000 * FAMILIES.index(family))
    out = []
    for n, off, ln in code_rate_windows():
        pos = peak_positions(ln)
        if family in ('zero', 'all_nan'):
            pos = {}
        elif family == 'neg_zero':
            pos = {k: v for k, v in pos.items() if k == 'middle'}
            pos['none'] = ()
        elif family == 'mixed':
            pos = {k: v for k, v in pos.items() if not k.startswith('tie')}
        elif family in ('one_inf', 'two_inf'):
            pos = {k: v for k, v in pos.items() if k in ('first', 'middle')}
        seen, uniq = set(), []                # distinct positions only (len 1: first = last = middle)
        for name, p in list(pos.items()) or [('none', ())]:
            if p not in seen:
                seen.add(p)
                uniq.append((name, p))
        batches = [[uniq[(i + j) % len(uniq)] for j in range(3)] for i in range(0, len(uniq), 3)] + [uniq[:1]]
        for chunk in batches:
            wins = [code_rate_window(rs, family, n, off, ln, p) for _, p in chunk]
            out.append((n, off, ln, '+'.join(nm for nm, _ in chunk), np.stack([w[0] for w in wins]), [w[1] for w in wins]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# centres
# ------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf for the magnitudes used here: the product of two fp32 values and the sum with a small integer are exact in float64."""
    return f32(float(f32(a)) * float(f32(b)) + float(f32(c)))


def centres_model(sig, W, op, spSym, offset, capacity, nthreads):
    """findCentres, CU:78-146, one thread after the other.  -> (sym int32, cen int32, mag float32, tags): the three outputs with
    ceil(nthreads / 256) * 256 entries, CANARY where the kernel writes nothing; tags = the branches that were reached."""
    M, lenSig = sig.shape
    nent = (nthreads + 255) // 256 * 256
    sym = np.full(nent, CANARY, np.int32)
    cen = np.full(nent, CANARY, np.int32)
    mag = np.full(nent, CANARY_F32, np.float32)
    re, im = sig.real.astype(np.float64).tolist(), sig.imag.astype(np.float64).tolist()      # small integers: float64 is exact too
    spSym, offset = f32(spSym), f32(offset)
    tags = set()
    for x in range(nent):
        if x >= capacity:
            tags.add('canary')
            continue
        half = f32(W // 2)
        base = _fma32(f32(x), spSym, -half)
        arrayIdx = int(f32(base + offset))              # Python's int: truncation, without a range
        maxArrayIdx = arrayIdx + W
        offsetComp = int(offset)
        if arrayIdx < 0:
            tags.add('neg_start_frac' if float(offset) != int(offset) else 'neg_start')
            offsetComp -= arrayIdx
            arrayIdx = 0
        if maxArrayIdx > lenSig:
            if arrayIdx < lenSig:
                tags.add('cut_by_end')
            maxArrayIdx = lenSig
        maxArrayIdx -= arrayIdx
        if not arrayIdx < lenSig:
            tags.add('start_at_len' if arrayIdx == lenSig else 'sentinel')
            if arrayIdx >= 1 << 31:
                tags.add('beyond_int32')
            sym[x], cen[x], mag[x] = INT32_MIN, INT32_MIN, 0.0
            continue
        if arrayIdx == lenSig - 1:
            tags.add('start_last')
        maxVal, maxIdx, maxCentreIdx = 0.0, -1, -1
        ties_m = ties_k = nans = 0
        for m in range(M):
            for k in range(maxArrayIdx):
                a, b = re[m][arrayIdx + k], im[m][arrayIdx + k]
                tmp = a * a + b * b if op == 0 else (abs(a) if op == 1 else abs(b))
                if tmp != tmp:
                    nans += 1
                if tmp > maxVal:
                    maxVal, maxIdx, maxCentreIdx = tmp, m, k
                    ties_m = ties_k = 0
                    neg = (op == 1 and a < 0) or (op == 2 and b < 0)
                elif tmp == maxVal and maxIdx >= 0:
                    ties_m += m != maxIdx
                    ties_k += m == maxIdx
        if maxIdx < 0:
            tags.add('nan_only' if nans == M * maxArrayIdx and nans else ('zero_window' if not nans else 'nan_and_zero'))
        else:
            if ties_m:
                tags.add('tie_filters')
            if ties_k:
                tags.add('tie_positions')
            if nans:
                tags.add('nan_skipped')
            if neg:
                tags.add('negative_maximum')
        sym[x] = maxIdx
        cen[x] = int(f32(f32(base + f32(maxCentreIdx)) + f32(offsetComp)))
        mag[x] = maxVal
    return sym, cen, mag, tags


CENTRES_LEN = (1, 6, 37, 300)
CENTRES_M = (1, 2, 5)
CENTRES_W = (1, 3, 7, 9)
CENTRES_OP = (0, 1, 2)
SIG_PATTERNS = ('random', 'constant', 'rows_equal', 'rows_constant', 'zero', 'nan_some', 'nan_all', 'negative')


def centres_signal(rs, pattern, M, lenSig):
    """Small-integer components: every magnitude is exact."""
    sig = (rs.randint(-3, 4, (M, lenSig)) + 1j * rs.randint(-3, 4, (M, lenSig))).astype(np.complex64)
    if pattern == 'constant':                  # every filter and every position ties: filter 0, position 0 win
        sig[:] = 2 - 2j
    elif pattern == 'rows_equal':              # ties between the filters only
        sig[:] = (np.arange(lenSig) % 7 + 1) * (1 + 1j)
    elif pattern == 'rows_constant':           # ties between the positions only: the last filter's first position wins
        sig[:] = ((np.arange(M) + 1) * (1 - 1j))[:, None]
    elif pattern == 'zero':
        sig[:] = 0
    elif pattern == 'nan_some':                # NaN beside finite positive values, and windows of NaN and zeros alone
        sig[:, ::2] = complex(np.nan, np.nan)
        sig[:, lenSig // 2:lenSig // 2 + 12] = 0
        sig[0, lenSig // 2:lenSig // 2 + 12:2] = complex(np.nan, np.nan)
    elif pattern == 'nan_all':
        sig[:] = complex(np.nan, np.nan)
    elif pattern == 'negative':                # the largest |component| is a negative one
        sig[:] = (rs.randint(-1, 2, (M, lenSig)) + 1j * rs.randint(-1, 2, (M, lenSig)))
        sig[M - 1, ::2] = -9 - 8j
    return sig


def centres_variants(lenSig, W):
    """(name, spSym, offset, capacity, nthreads, tags the case is named for)"""
    half = W // 2
    v = [
        # x = 0 starts at -half; 2 samples per symbol: the windows overlap, the last ones are cut by the end (W >= 3)
        ('dense', 2.0, 0.0, 256, 256, {'neg_start', 'cut_by_end'} if half else set()),
        # a fractional offset below W / 2 (a start in (-1, 0) truncates to 0: the branch needs half >= 2); capacity above nthreads: the
        # whole last workgroup writes, the canary starts at capacity
        ('fractional', 2.5, 0.75, 300, 257, {'canary'} | ({'neg_start_frac'} if half >= 2 else set())),
        # more samples per symbol than samples: every x >= 1 is a sentinel; capacity below nthreads
        ('sparse', float(lenSig + W), 0.25, 100, 256, {'sentinel', 'canary'}),
        # one thread, one entry
        ('single', 3.0, 1.0, 1, 1, {'canary'}),
    ]
    # a window that starts at lenSig - 1 (start lenSig - 0.5) and one that starts exactly at lenSig: 2 x - half + offset = target
    for name, target, frac, tag in (('at_last', lenSig - 1, 0.5, 'start_last'), ('at_len', lenSig, 0.0, 'start_at_len')):
        v.append((name, 2.0, float((target + half) % 2) + frac, 256, 256, {tag}))
    return v


def centres_cases(lenSig, op, seed=0):
    """Every M x W of the table with every variant; the signal patterns rotate so that each meets each variant."""
    rs = np.random.RandomState(seed + 10 * lenSig + op)
    out, i = [], 0
    for M in CENTRES_M:
        for W in CENTRES_W:
            for name, spSym, offset, capacity, nthreads, tags in centres_variants(lenSig, W):
                for rep in range(2):
                    pattern = SIG_PATTERNS[i % len(SIG_PATTERNS)]
                    i += 3                      # 3 and 8 are coprime: every pattern comes up; 2 per variant, 6 variants: they drift
                    out.append(dict(name=f'{name}-{pattern}-M{M}-W{W}', sig=centres_signal(rs, pattern, M, lenSig), W=W, op=op, spSym=spSym,
                                    offset=offset, capacity=capacity, nthreads=nthreads, pattern=pattern, tags=set(tags)))
    return out


# the conversion overflow: x * spSym passes 2^31 from x = 72 on
OVERFLOW_CASE = dict(lenSig=64, M=2, W=7, spSym=3e7, offset=0.5, capacity=256, nthreads=256)
