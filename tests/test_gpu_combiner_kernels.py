"""The soft combiner's kernels (pycusdr_amd/csrc/combine_kernels.hpp) at the edges of their launch arithmetic, each against a
plain exact reference (tests/combiner_model.py, held to the definition and to numpy by test_combiner_model.py).  Every
comparison is ``==`` / ``array_equal``; there is no tolerance in this file.

What decides the shapes (cmb_enqueue_xcorr, combine_api.hpp): N = 2^ceil(log2 n) lags, NW = max(N / 32, 1) slave words,
gx = ceil(NW / 256) workgroups along the lags, tiles = ceil(ceil(min(m, n) / 32) / 64) tiles of 64 master words,
gy = min(1024 / gx, tiles): a workgroup of k_cmb_xcorr walks more than one tile only when gx * tiles > 1024, that is from
N = 2^18 with more than 65 536 master bits on.  The peak stages take 4096 lags per workgroup (16 per thread, lag
j * 256 + thread in register slot j) and merge 15 candidates per workgroup, at most 3840 at the limit of 2^20 lags."""
import numpy as np
import pytest

import combiner_common as cc
import combiner_model as cm

pytestmark = pytest.mark.gpu

VM, WEIGHT = 15.0, 1.2


def _bits(rs, n):
    return rs.randint(0, 2, n).astype(np.uint8)


def _check_xcorr(a, b, want=None):
    from pycusdr_amd import mfbank
    got = mfbank.bit_xcorr(a, b)
    if want is None:
        want = cm.exact_xcorr(a, b)
    assert got.dtype == np.int32 and got.shape == want.shape, (len(a), len(b), got.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (len(a), len(b), bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    return got


# ---- the correlation -----------------------------------------------------------------------------------------------------------
def test_xcorr_of_one_word_and_below():
    """NW = 1: alignbit(S[0], S[0], r) is the whole circular wrap, and below 32 lags the slave word is the n bits repeated with
    period N.  Every slave length from one bit to beyond a word, and around two words, against masters of one bit, around the
    word borders, of the slave's length and longer (only the first n bits count)."""
    rs = np.random.RandomState(201)
    for n in list(range(1, 41)) + [63, 64, 65]:
        a = _bits(rs, n)
        for m in (1, 2, 15, 16, 17, 31, 32, 33, 65, n, n + 1):
            _check_xcorr(a, _bits(rs, m))


@pytest.mark.parametrize('n', [8191, 8192, 8193, 16384])
def test_xcorr_at_the_grid_borders(n):
    """n <= 8192 is NW = 256, the last shape with gx = 1; 8193 and 16384 are the first with gx = 2.  2047, 2048 and 2049 master
    bits put the end of the master before, at and behind the border of the first tile of 64 words (a short second tile of one
    word with one valid bit); m = n is every tile full."""
    rs = np.random.RandomState(202)
    a = _bits(rs, n)
    for m in (2047, 2048, 2049, n):
        _check_xcorr(a, _bits(rs, m))


def test_xcorr_loops_once_in_one_row_of_workgroups():
    """n = 131 073, m = 65 537: N = 2^18, gx = 32, gy = 32 and 33 tiles.  Only the workgroups of blockIdx.y == 0 make a second
    pass, over one master word that holds one valid bit: wend = 1, the barrier and the re-staging after a full first tile."""
    rs = np.random.RandomState(203)
    _check_xcorr(_bits(rs, 131073), _bits(rs, 65537))


@pytest.mark.parametrize('n, m', [(1 << 18, 1 << 18), ((1 << 18) - 3, (1 << 18) + 77)])
def test_xcorr_loops_evenly(n, m):
    """128 tiles on gy = 32: four passes per workgroup, acc[] carried through all of them.  With n = 2^18 - 3 the length that
    counts is n, not m: the last word is masked, with live master bits behind the mask."""
    rs = np.random.RandomState(204)
    _check_xcorr(_bits(rs, n), _bits(rs, m))


def test_xcorr_of_degenerate_streams_in_the_loop():
    """N = 2^18, four passes.  All-ones against all-ones: every lag is 2^18, every partial sum as large as it gets.  An all-zero
    slave or master: nothing is added (the v != 0 skip) and x stays zero.  A master of a single one-bit at position 65 536 (the
    first word of the second pass of blockIdx.y == 0): x[k] = a[(65 536 + k) mod N], the slave rotated."""
    N = 1 << 18
    rs = np.random.RandomState(205)
    ones, zeros, a = np.ones(N, np.uint8), np.zeros(N, np.uint8), _bits(rs, N)
    _check_xcorr(ones, ones, np.full(N, N, np.int64))
    _check_xcorr(zeros, a, np.zeros(N, np.int64))
    _check_xcorr(a, zeros, np.zeros(N, np.int64))
    one = zeros.copy()
    one[65536] = 1
    _check_xcorr(a, one, np.roll(a, -65536).astype(np.int64))


def test_xcorr_at_the_limit_of_2_20_bits():
    """n = m = 2^20 (CMB_MAX_BITS): gx = 128, gy = 8, 64 passes per workgroup.  Reference: the float64 FFT form rounded, which
    is held to lie within 0.01 of integers here (about 1e-11 in practice), and direct int64 dot products at the first lags, the
    lags around a word, the last lag and 64 random ones."""
    n = 1 << 20
    rs = np.random.RandomState(206)
    a, b = _bits(rs, n), _bits(rs, n)
    xf = np.fft.irfft(np.fft.rfft(a.astype(np.float64)) * np.conj(np.fft.rfft(b.astype(np.float64))), n)
    want = np.rint(xf)
    assert np.abs(xf - want).max() < 0.01
    got = _check_xcorr(a, b, want.astype(np.int64))
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    for k in [0, 1, 31, 32, 33, n - 1] + [int(k) for k in rs.randint(0, n, 64)]:
        assert int(got[k]) == int(np.dot(np.roll(a64, -k), b64)), k


# ---- peaks and decision ----------------------------------------------------------------------------------------------------------
def _check_peaks(x, n=None, master_len=None, min_length=1, vm=VM):
    """mfbank.combine_peaks (k_cmb_init, k_cmb_top_seg, k_cmb_decide, k_cmb_finish as a call launches them) on x against
    top_peaks, decision_exact and decide_state: the fifteen values and the first one's lag, cond bit for bit, and the
    bookkeeping.  Returns the slave's record and the whole result."""
    from pycusdr_amd import mfbank, softCombiner as sc
    x = np.asarray(x)
    n = len(x) if n is None else n
    master_len = n if master_len is None else master_len
    res = mfbank.combine_peaks(x, n, master_len, vm, min_length)
    val, idx0 = sc.top_peaks(x)
    want = cm.decide_state(val, idx0, n, master_len, min_length, vm)
    assert len(res['slaves']) == 1
    r = res['slaves'][0]
    what = (len(x), n, master_len, min_length, vm, r, want)
    assert r['evaluated'] == 1
    assert r['val'].dtype == np.int32 and np.array_equal(r['val'], val), what
    assert r['idx0'] == idx0, what
    assert r['cond'] == want['cond'], what
    assert (r['matched'], r['avail'], r['lc_after'], res['status']) == (want['matched'], want['avail'], want['lc_after'], want['status']), what
    assert res['matched'] == ([0] if want['status'] == cm.COMBINED else []), what
    assert res['out_len'] == (0 if want['status'] == cm.NOTHING else want['lc_after']), what
    return r, res


@pytest.mark.parametrize('nlags', [16, 4096, 4097, 8192, 1 << 16, 1 << 20])
def test_peaks_of_random_correlations(nlags):
    """Values in [0, hi]: at hi = 1, 3 and 40 nearly every one of the fifteen rounds, in both stages, is decided by the index in
    the key; at 2^20 hardly any.  One segment short and full, one lag into a second segment, two segments, sixteen, and 256
    segments: 3840 candidates, fifteen of the sixteen register slots of k_cmb_decide."""
    rs = np.random.RandomState(210 + nlags % 97)
    for hi in (1, 3, 40, 1 << 20):
        x = rs.randint(0, hi + 1, nlags)
        for vm in (15.0, 0.1):
            _check_peaks(x, master_len=nlags // 2 + 1, vm=vm)


NL = 3 * 4096 + 5           # three segments and a fourth of five lags


@pytest.mark.parametrize('lo, hi', [(4096 + 300, 4096 + 300 + 256), (4096 + 300, 4096 + 301), (63, 64), (4095, 4096), (0, NL - 1),
                                     (4096 + 63, 4096 + 64), (2 * 4096 - 1, 2 * 4096), (255, 256), (3 * 4096 - 1, 3 * 4096)])
def test_two_equal_maxima_the_lower_lag_wins(lo, hi):
    """The tie rule is ~index in the key.  Two equal maxima in two register slots of one thread (lags 256 apart), in neighbouring
    lanes, across the border of two waves, of two threads' slots, of two segments (decided in k_cmb_decide), and at the two ends."""
    rs = np.random.RandomState(220)
    x = rs.randint(0, 50, NL)
    x[[lo, hi]] = 1000
    r, _ = _check_peaks(x, vm=0.1)
    assert r['idx0'] == lo and list(r['val'][:3]) == [1000, 1000, 49]
    x[lo] = 999                                      # and the larger value wins whatever its index
    r, _ = _check_peaks(x, vm=0.1)
    assert r['idx0'] == hi and list(r['val'][:3]) == [1000, 999, 49]


def test_many_equal_maxima():
    """Fifteen equal maxima, one in each of fifteen segments (every candidate list hands over one, the merge orders them by
    lag); forty equal maxima inside one segment, which can hand over only fifteen -- all fifteen winners -- with smaller values
    elsewhere; and fifteen distinct winners that all lie in the last, partly filled segment."""
    rs = np.random.RandomState(221)
    x = rs.randint(0, 50, 16 * 4096)
    at = [s * 4096 + (s * 977) % 4096 for s in range(1, 16)]
    x[at] = 777
    r, _ = _check_peaks(x)
    assert r['idx0'] == at[0] and list(r['val']) == [777] * 15 and r['cond'] == 777.0 and not r['matched']
    x = rs.randint(0, 50, NL)
    at = 4096 + rs.choice(4096, 40, replace=False)
    x[at] = 777
    r, _ = _check_peaks(x)
    assert r['idx0'] == at.min() and list(r['val']) == [777] * 15
    x = rs.randint(0, 50, 2 * 4096 + 1000)
    at = 2 * 4096 + rs.choice(1000, 15, replace=False)
    x[at] = 1000 + rs.permutation(15) * 7
    r, _ = _check_peaks(x, vm=0.1)
    assert r['idx0'] == at[np.argmax(x[at])] and list(r['val']) == sorted(x[at], reverse=True)


def test_thin_correlations():
    """All zero: the real keys of value 0 (their low half is ~index, never 0) compete with the padding key 0; lag 0 wins,
    val = 0, cond = 0 and 0 > 0 does not match.  Then exactly 1, 2, 14 and 15 non-zero lags, none of them at lag 0."""
    for nlags in (16, 5000, 1 << 16):
        r, res = _check_peaks(np.zeros(nlags, np.int64))
        assert r['idx0'] == 0 and not r['val'].any() and r['cond'] == 0.0 and r['matched'] == 0 and res['status'] == cm.MASTER_ONLY
    rs = np.random.RandomState(222)
    for nlags in (16, 4097, 1 << 16):
        for count in (1, 2, 14, 15):
            x = np.zeros(nlags, np.int64)
            at = 1 + rs.choice(nlags - 1, count, replace=False)
            x[at] = rs.randint(1, 4, count)
            for vm in (15.0, 0.1):
                r, _ = _check_peaks(x, vm=vm)
                assert np.count_nonzero(r['val']) == count and r['idx0'] == at[x[at] == x[at].max()].min()


@pytest.mark.parametrize('c', [1, 13, 65536, 1 << 20])
def test_the_threshold_is_strict(c):
    """A flat correlation: mean = c exactly, every deviation 0, cond == c == val[0], and v[0] > cond is false.  Two lags at
    c + 1 leave val[2:] flat and match."""
    for nlags in (16, 4096 + 17):
        x = np.full(nlags, c, np.int64)
        r, res = _check_peaks(x)
        assert r['cond'] == float(c) and r['val'][0] == c and r['matched'] == 0 and r['idx0'] == 0 and res['status'] == cm.MASTER_ONLY
        x[[5, nlags - 2]] = c + 1
        r, res = _check_peaks(x)
        assert r['cond'] == float(c) and r['val'][0] == c + 1 and r['matched'] == 1 and r['idx0'] == 5 and res['status'] == cm.COMBINED


def test_bookkeeping_of_a_matched_slave():
    """One clear peak at lag p of 8192: avail = max(0, min(Lc, n - p)) at min_length, one below it (the call ends with nothing,
    out_len 0), with the peak in the zero padding behind the slave's n bits (avail clamps to 0), shorter than the master (Lc
    shrinks) and longer (Lc stays)."""
    rs = np.random.RandomState(223)
    x = rs.randint(0, 50, 8192)
    x[4000] = 100000
    r, res = _check_peaks(x, n=5000, master_len=3000, min_length=1000)
    assert (r['matched'], r['avail'], r['lc_after'], res['status'], res['out_len']) == (1, 1000, 1000, cm.COMBINED, 1000)
    r, res = _check_peaks(x, n=5000, master_len=3000, min_length=1001)
    assert (r['matched'], r['avail'], r['lc_after'], res['status'], res['out_len']) == (1, 1000, 3000, cm.NOTHING, 0)
    r, res = _check_peaks(x, n=8000, master_len=3000, min_length=1000)
    assert (r['matched'], r['avail'], r['lc_after'], res['status'], res['out_len']) == (1, 3000, 3000, cm.COMBINED, 3000)
    r, res = _check_peaks(x, n=8000, master_len=3000, min_length=3000)
    assert (r['avail'], res['status']) == (3000, cm.COMBINED)
    x[4000], x[6000] = 7, 100000
    r, res = _check_peaks(x, n=5000, master_len=3000, min_length=1)
    assert (r['matched'], r['idx0'], r['avail'], r['lc_after'], res['status'], res['out_len']) == (1, 6000, 0, 3000, cm.NOTHING, 0)
    r, res = _check_peaks(x, n=6000, master_len=3000, min_length=1)        # idx0 == n: nothing left either
    assert (r['avail'], res['status']) == (0, cm.NOTHING)
    r, res = _check_peaks(x, n=6001, master_len=3000, min_length=1)
    assert (r['avail'], r['lc_after'], res['status'], res['out_len']) == (1, 1, cm.COMBINED, 1)


def test_the_peak_seam_refuses_what_it_cannot_run():
    import ctypes as C
    from pycusdr_amd import _lib
    lib = _lib.load()
    R = _lib.CombineResult()
    x = np.zeros((1 << 20) + 1, np.int32)
    ptr = x.ctypes.data_as(C.c_void_p)
    assert lib.mfb_debug_combine_peaks(0, ptr, 0, 16, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, 0, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, 16, 0, VM, 1, C.byref(R)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, None, 16, 16, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, 16, 16, VM, 1, None) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, ptr, (1 << 20) + 1, 16, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_UNSUPPORTED
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, (1 << 20) + 1, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_UNSUPPORTED
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, 16, (1 << 20) + 1, VM, 1, C.byref(R)) == _lib.MFB_ERR_UNSUPPORTED
    x[15] = -1
    assert lib.mfb_debug_combine_peaks(0, ptr, 16, 16, 16, VM, 1, C.byref(R)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_combine_peaks(0, ptr, 15, 16, 16, VM, 1, C.byref(R)) == _lib.MFB_OK


# ---- whole calls -------------------------------------------------------------------------------------------------------------------
def _combiner(max_bits, weight=WEIGHT):
    from pycusdr_amd import mfbank, softCombiner as sc
    c = mfbank.Combiner(max_bits=max_bits)
    for v in (2, 3, 4):
        c.set_vote(v, *sc.vote_table(v, weight))
    return c


def _trust(rs, n):
    return rs.choice(np.array(cc.TRUST_REPS, dtype=np.int8), n)


def test_one_word_slaves_through_a_call():
    """Slaves of 16, 17, 31, 32 and 33 bits (NW = 1; 33 bits: the first with two words) that hold a twelve-bit master, alone and
    all three of a kind in one call, min_length = 8, at the reference's variance multiplier and at one that matches: the
    device's records, cond included, and votes equal the host back end's."""
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(230)
    c = _combiner(1 << 10)
    matched = 0
    for n in (16, 17, 31, 32, 33):
        m = rs.randint(0, 2, 12).astype(np.int8)
        m[[0, 5, 11]] = 1
        slaves = []
        for off in (0, 3, n - 12):
            b = np.zeros(n, np.int8)
            b[off:off + 12] = m
            slaves.append((b, _trust(rs, n)))
        t = _trust(rs, 12)
        for vm in (VM, 0.5):
            for sl in ([slaves[0]], [slaves[1]], [slaves[2]], slaves):
                got = c.combine(m, t, sl, vm, 8)
                assert all(r['evaluated'] for r in got['slaves'])
                cc.same_core(got, sc.combine_host(m, t, sl, vm, WEIGHT, 8))
                matched += len(got['matched'])
    assert matched > 0
    c.close()


def test_calls_at_the_limit_of_2_20_bits():
    """A 2^20-bit slave that holds a 2^19-bit master at lag 12 345: 32 passes of the correlation, 256 segments and 3840
    candidates of the peak stages, in one call.  Then the same behind a 2^18-bit slave that the master overruns (150 001
    of its bits fit): Lc shrinks on the device between the two correlations, and the second one, whose grid was sized for 2^19
    master bits, loops over the 150 001 that are left.  Both equal the host back end, without its help."""
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(231)
    Lm, n1, n0, keep = 1 << 19, 1 << 20, 1 << 18, 150001
    m, t = rs.randint(0, 2, Lm).astype(np.int8), _trust(rs, Lm)
    big = rs.randint(0, 2, n1).astype(np.int8)
    big[12345:12345 + Lm] = m ^ (rs.random_sample(Lm) < 0.03)
    small = rs.randint(0, 2, n0).astype(np.int8)
    small[n0 - keep:] = m[:keep] ^ (rs.random_sample(keep) < 0.03)
    s_big, s_small = (big, _trust(rs, n1)), (small, _trust(rs, n0))
    hip = sc.SoftCombiner(cc.conf_of(), backend='hip')
    for slaves, idx0, lc in (([s_big], [12345], [Lm]), ([s_small, s_big], [n0 - keep, 12345], [keep, keep])):
        got = hip.combine(m, t, slaves)
        assert got['status'] == sc.COMBINED and got['matched'] == list(range(len(slaves)))
        assert [r['idx0'] for r in got['slaves']] == idx0 and [r['lc_after'] for r in got['slaves']] == lc
        cc.same_core(got, sc.combine_host(m, t, slaves, VM, WEIGHT, 200))
    assert hip.host_fallbacks == 0
    hip.close()


def _class_values():
    """The trust bytes of cc.TRUST_REPS by the class the vote sees: {< -1, -1, 0, > 0}."""
    reps = np.array(cc.TRUST_REPS)
    return [reps[reps < -1], reps[reps == -1], reps[reps == 0], reps[reps > 0]]


def _enumerated_streams(rs, K, offs, prefix=4000, tail=60):
    """A master and K slaves: a random prefix that the slaves share (5 % of the bits flipped), which carries the alignment, then
    8^(K+1) columns of which column e has the state e -- voter v's code is digit v of e in base 8 -- with each class's trust
    byte going round the values that cc.TRUST_REPS has for it."""
    E = 8 ** (K + 1)
    e = np.arange(E)
    cls_vals = _class_values()
    head = rs.randint(0, 2, prefix).astype(np.int8)
    streams = []
    for v in range(K + 1):
        code = (e >> (3 * v)) & 7
        tr = np.zeros(E, dtype=np.int8)
        for cl, vals in enumerate(cls_vals):
            cols = np.flatnonzero((code & 3) == cl)
            tr[cols] = vals[(np.arange(len(cols)) + v) % len(vals)]
        bits = (code >> 2).astype(np.int8)
        if v == 0:
            streams.append((np.r_[head, bits], np.r_[_trust(rs, prefix), tr]))
        else:
            off = offs[v - 1]
            b = np.r_[rs.randint(0, 2, off).astype(np.int8), head ^ (rs.random_sample(prefix) < 0.05), bits, rs.randint(0, 2, tail).astype(np.int8)]
            streams.append((b.astype(np.int8), np.r_[_trust(rs, off + prefix), tr, _trust(rs, tail)]))
    return streams[0], streams[1:]


@pytest.mark.parametrize('weight', cc.WEIGHTS)
def test_every_entry_of_the_vote_tables(weight):
    """k_cmb_vote with one, two and three matched slaves on streams that hold every column state exactly once, in order: the
    output over those columns is the vote table, entry for entry, and the states as the device saw them -- the slaves cut at
    the idx0 it reported -- are all 8^(K+1)."""
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(232)
    c = _combiner(1 << 14, weight)
    P = 4000
    for K in (1, 2, 3):
        E = 8 ** (K + 1)
        offs = [17, 1000, 333][:K]
        (m, t), slaves = _enumerated_streams(rs, K, offs, prefix=P)
        for v, (_, tr) in enumerate([(m, t)] + slaves):
            o = 0 if v == 0 else offs[v - 1]
            assert set(tr[o + P:o + P + E].tolist()) == set(cc.TRUST_REPS)
        res = c.combine(m, t, slaves, VM, 200)
        assert res['status'] == sc.COMBINED and res['matched'] == list(range(K)) and len(res['bits']) == P + E
        idx0 = [r['idx0'] for r in res['slaves']]
        assert idx0 == offs
        L = P + E
        states = sc.column_states([m] + [b[o:o + L] for (b, _), o in zip(slaves, idx0)], [t] + [tr[o:o + L] for (_, tr), o in zip(slaves, idx0)])
        assert np.array_equal(states[P:], np.arange(E)) and len(np.unique(states[P:])) == E
        tb, tt = sc.vote_table(K + 1, weight)
        assert np.array_equal(res['bits'][P:], tb) and np.array_equal(res['trust'][P:], tt), (weight, K)
        assert np.array_equal(res['bits'], tb[states]) and np.array_equal(res['trust'], tt[states]), (weight, K)
    c.close()
