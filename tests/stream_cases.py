"""The case table of the stream-stage edge tests: every case names the branch of csrc/stream_kernels.hpp it is built for and states,
as assertions on the MODEL's results alone (``reach``), that it gets there -- tests/test_stream_model.py runs that without a GPU, so
the device comparison in tests/test_gpu_stream_edges.py cannot pass vacuously.  A case is a geometry (the arguments of
``StreamModel`` / ``MFBank.set_stream_stages``), a record capacity and a list of steps:
    ('seed', post, end, ring)   MFBank.stream_seed
    ('reseed',)                 seed with the host code's state now (what a caller does behind a block that went to the host)
    ('batch', blocks)           one device call on blocks = [(count, sym, cen, mag), ...]
``drive`` runs the steps through the model and, given a bank, through the device in lockstep; ``check_batch`` holds a batch's
device records to the model's results, everything with np.array_equal."""
import functools

import numpy as np

from pycusdr_amd.demodulator.demodulator_base import Demodulator
from stream_model import StreamModel, make_blocks, MAX_HITS, EDGE_CANDS

LUT8 = np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=np.uint8)
NONE = np.zeros(0, np.uint8)
DEVICE = ('device-expected', 'repaired +1', 'repaired -1')


def nrzs_lut(rows=16, succ=4):
    """symbolLUT[s][0 | 1][q]: successors of s that mean a one (odd steps) / a zero (even steps); steps of 0 and of more than
    2 succ are impossible transitions."""
    s, q = np.arange(rows)[:, None], np.arange(succ)[None, :]
    return np.stack(((s + 1 + 2 * q) % rows, (s + 2 + 2 * q) % rows), axis=1).astype(np.int32)


def nrzs_lut_last_slot():
    """16 x 2 x 64 = 2048 entries (the LDS copy's limit); the only match sits in the last successor slot, -1 is no symbol."""
    lut = np.full((16, 2, 64), -1, dtype=np.int32)
    lut[:, 0, 63] = (np.arange(16) + 1) % 16
    lut[:, 1, 63] = (np.arange(16) + 3) % 16
    return lut


def the_lut(mode):
    return LUT8 if mode == 'lut' else nrzs_lut()


def sp(count, start, after, slip=0, plant=None):
    return {'count': count, 'start': start, 'after': after, 'slip': slip, 'plant': plant or {}}


def aft(mode, npost):
    """centres behind the window that leave `npost` BITS there (an NRZ-S bit needs its successor)"""
    return npost + (mode == 'nrzs')


class Case:
    def __init__(self, name, cap, steps, reach, log2N=13, overlap_samples=1 << 10, o=20, match_thr=10, err_thr=1000, lut=LUT8,
                 templates=(), thresholds=(), nOv=0):
        self.name, self.cap, self.steps, self.reach, self.log2N = name, cap, steps, reach, log2N
        self.kw = dict(N=1 << log2N, overlap_samples=overlap_samples, o=o, match_thr=match_thr, err_thr=err_thr, lut=lut,
                       templates=templates, thresholds=thresholds, nOv=nOv)

    def blocks(self, rs, specs, p_err=0.0):
        return make_blocks(rs, self.kw['lut'], specs, self.kw['N'], self.kw['overlap_samples'], self.cap, p_err)


def tags(batches):
    return [r['tag'] for res in batches for r in res]


# ---- A12 / A13 -------------------------------------------------------------------------------------------------------------------
def second_stride(mode, cap):
    """k_stream_align's strided sweep: more than 4096 symbols per block, so the first-start / first-end minima, the irregular flag
    and the mismatch count come from its later trips."""
    o = 20 if cap == 8192 else 31
    lut, a = the_lut(mode), aft(mode, 40)
    c = Case(f'second_stride-{mode}-{cap}', cap, None, None, log2N=15, o=o, match_thr=o // 2, lut=lut)
    same = {x + 1: (lambda s, x=x: s[x]) for x in (7, 4095, 4096, cap - 4097)}      # impossible NRZ-S steps on group borders
    specs = [sp(cap, 40, a), sp(cap, 40, a, slip=1), sp(cap - 1, 43, a), sp(cap, 5000, aft(mode, 35)),
             sp(cap, 40, a, slip=-1, plant=same if mode == 'nrzs' else None), sp(cap - 2, 40, a),
             sp(cap, 40, a, plant={cap - 2100: lut.shape[0]}), sp(cap, 40, a), sp(cap - 3, 40, a, slip=1)]
    b = c.blocks(np.random.RandomState(cap + (mode == 'nrzs')), specs)
    c.steps = [('seed', NONE, NONE, None), ('batch', b[:5]), ('batch', b[5:])]

    def reach(batches):
        t = tags(batches)
        assert 'repaired +1' in t and 'repaired -1' in t, t
        assert all(r['count'] > 4096 for res in batches for r in res)
        assert batches[0][3]['start0'] == 5000 and t[3] in DEVICE, t              # the first start comes from the second trip
        assert t[6] == 'irregular' and batches[1][1]['host_error'], t            # the index outside the LUT sits above 4096 only
        assert t[7] == 'irregular' and t[8] in DEVICE, t
        if mode == 'nrzs':
            assert batches[0][4]['noerr'] >= 4 and t[4] in DEVICE, (batches[0][4]['noerr'], t)
    c.reach = reach
    return c


def count_tails(mode):
    """A record capacity that is no multiple of four; counts from the capacity down to capacity - 3; an index outside the LUT at
    count - 1 (NRZ-S: only ever a successor) and at count - 2."""
    cap, lut, a = 2047, the_lut(mode), aft(mode, 30)
    c = Case(f'count_tails-{mode}', cap, None, None, lut=lut)
    rows = lut.shape[0]
    specs = [sp(cap, 25, a), sp(cap - 1, 25, a, slip=1), sp(cap - 2, 26, a), sp(cap - 3, 25, a), sp(cap, 25, a, plant={cap - 1: rows}),
             sp(cap - 1, 25, a), sp(cap - 1, 25, a, plant={cap - 3: rows}), sp(cap, 25, a), sp(cap, 25, a)]
    c.steps = [('seed', NONE, NONE, None), ('batch', c.blocks(np.random.RandomState(3 + (mode == 'nrzs')), specs))]

    def reach(batches):
        t = tags(batches)
        assert all(x in DEVICE for x in t[:4]) and 'repaired +1' in t[:4] and 'repaired -1' in t[:4], t
        assert t[4:8] == ['irregular'] * 4 and batches[0][6]['host_error'], t
        # (NRZ-S: the index at count - 1 is only ever a successor -- the host code sees an impossible transition, the device's
        # precondition fails)
        assert (batches[0][4]['host_error'] is None) == (mode == 'nrzs'), batches[0][4]['host_error']
        assert batches[0][5]['host_error'] is None and t[8] in DEVICE, t
    c.reach = reach
    return c


def tiny(mode):
    """Counts of 0, 1 and o + 1; a window of exactly o + 1 symbols (the host's) and of o + 2 (the device's)."""
    o, lut = 3, the_lut(mode)
    a = aft(mode, 6)
    c = Case(f'tiny-{mode}', 64, None, None, o=o, match_thr=1, lut=lut)
    specs = [sp(40, 6, a), sp(0, 0, 0), sp(1, 0, 0), sp(o + 1, 1, 1), sp(6 + o + 1 + a, 6, a), sp(40, 6, a), sp(6 + o + 2 + a, 6, a), sp(40, 6, a)]
    c.steps = [('seed', NONE, NONE, None), ('batch', c.blocks(np.random.RandomState(5), specs))]

    def reach(batches):
        t, res = tags(batches), batches[0]
        assert t[0] in DEVICE and t[1:6] == ['irregular'] * 5 and t[6] in DEVICE and t[7] in DEVICE, t
        assert res[4]['host_error'] is None and res[4]['nwin'] == o + 1 and res[6]['nwin'] == o + 2
        assert res[5]['ok'] and res[5]['host_error'] is None          # regular itself: the host's because its predecessor was
    c.reach = reach
    return c


def offset_limits(mode, o):
    """overlap_offset at its limits: the ends of the three thread ranges, the extents of p_post / p_end / s_near."""
    lut = the_lut(mode)
    c = Case(f'offset_limits-{mode}-{o}', 160, None, None, o=o, match_thr=max(o - 1, 0), lut=lut)
    slips = {2: 1, 5: -1, 7: 1, 10: -1}
    specs = [sp(150 - (b % 3), o + 1 + 2 * (b % 2), aft(mode, o + 1 + 3 * (b % 2)), slip=slips.get(b, 0)) for b in range(13)]
    c.steps = [('seed', NONE, NONE, None), ('batch', c.blocks(np.random.RandomState(100 * o + (mode == 'nrzs')), specs))]

    def reach(batches):
        t = tags(batches)
        assert all(x in DEVICE for x in t), t
        assert min(r['start0'] for r in batches[0]) == o + 1 and min(r['prev_npost'] for r in batches[0][1:]) == o + 1
        if o >= 2:
            assert 'repaired +1' in t and 'repaired -1' in t, t
            assert any(r['tag'] == 'repaired -1' and r['start0'] == o + 1 for r in batches[0]), t      # the window then starts at o
    c.reach = reach
    return c


def tails_seed():
    """The carry's tail at its lengths: post of 0, 1, o - 1, o and o + 1 bits in front of a slipped block, end of o and o + 1
    bits, an empty seed."""
    o = 20
    c = Case('tails_seed', 200, None, None, o=o)
    A, B, C = c.blocks(np.random.RandomState(21), [sp(190, 25, 40), sp(190, 25, 40, slip=1), sp(190, 25, 40)])
    m = StreamModel(**c.kw)
    m.seed(NONE, NONE)
    ra = m.batch([A])[0]
    post, end = ra['post'], ra['end']
    c.steps = []
    for k in (0, 1, o - 1, o, o + 1, 40):
        c.steps += [('seed', post[:k], end, None), ('batch', [B, C])]
    c.steps += [('seed', post, end[1:], None), ('batch', [B, C]), ('seed', post, NONE, None), ('batch', [B, C]),
                ('seed', NONE, NONE, None), ('batch', [B, C])]

    def reach(batches):
        t = [res[0]['tag'] for res in batches]
        assert t[0] == 'device-expected' and t[1] == t[2] == 'raised' and t[3] == 'irregular', t
        assert t[4] == t[5] and t[4] in ('repaired +1', 'repaired -1') and t[6] == t[7] == 'irregular' and t[8] == 'device-expected', t
        assert all(res[1]['tag'] in ('repaired +1', 'repaired -1') and res[1]['tag'] != t[4] for res in batches), tags(batches)
        assert batches[2][0]['host_logged']
    c.reach = reach
    return c


def tails_batch(mode):
    """The tail branches inside a batch, one by one: the previous block's npost of 0 (NRZ-S), 1, o - 1, o, o + 1; a start index of
    o and of o + 1; npost of this block at the record's 512 bits and one beyond."""
    o, lut = 20, the_lut(mode)
    c = Case(f'tails_batch-{mode}', 800, None, None, o=o, lut=lut)
    n, st, a = 700, 25, aft(mode, 40)
    specs = [sp(n, st, aft(mode, 1)), sp(n, st, aft(mode, o - 1), slip=1), sp(n, st, aft(mode, o)), sp(n, st, aft(mode, o + 1)),
             sp(n, st, a, slip=1), sp(n, o, a), sp(n, o + 1, a), sp(n, st, 512), sp(n, st, 513), sp(n, st, a), sp(n, st, aft(mode, 0)), sp(n, st, a, slip=1),
             sp(n, st, a)]
    c.steps = [('seed', NONE, NONE, None), ('batch', c.blocks(np.random.RandomState(31 + (mode == 'nrzs')), specs))]

    def reach(batches):
        t, res = tags(batches), batches[0]
        assert [r['prev_npost'] for r in res[1:5]] == [1, o - 1, o, o + 1]
        assert t[1] == t[2] == 'raised' and t[3] == 'irregular' and t[4] in ('repaired +1', 'repaired -1'), t
        assert res[2]['host_logged'] and res[3]['host_error'] is None
        assert t[5] == 'irregular' and res[5]['start0'] == o and t[6] in DEVICE and res[6]['start0'] == o + 1, t
        assert t[7] in DEVICE and t[8] == 'irregular' and t[9] in DEVICE and res[9]['prev_npost'] == 513 - (mode == 'nrzs'), t
        if mode == 'lut':
            assert res[7]['npost'] == 512 and t[10] == 'irregular' and res[10]['host_error'], t      # no centre behind the window
        else:
            assert res[7]['npost'] == 511 and t[10] in DEVICE and res[10]['npost'] == 0, t
            assert t[11] == 'device-expected' and res[11]['prev_npost'] == 0, t                          # p_npost == 0: nothing compared
    c.reach = reach
    return c


def tails_noerr(above):
    """NRZ-S: a planted slip with exactly err_thr impossible transitions (repaired) and with err_thr + 1 (not touched)."""
    lut = nrzs_lut()
    same = {x + 1: (lambda s, x=x: s[x]) for x in (50, 77, 90)}
    specs = [sp(190, 25, 41), sp(190, 25, 41, slip=1, plant=same), sp(190, 25, 41)]
    blocks = make_blocks(np.random.RandomState(41), lut, specs, 1 << 13, 1 << 10, 200)
    ns = type('L', (), {'symbolLUT': lut.astype(np.int64)})
    noerr = len(Demodulator.extractBitsNRZs(ns, None, blocks[1][1][:190].astype(np.int64))[1])
    c = Case(f'tails_noerr-{"above" if above else "equal"}', 200, [('seed', NONE, NONE, None), ('batch', blocks)], None,
             err_thr=noerr - 1 if above else noerr, lut=lut)

    def reach(batches):
        t, r = tags(batches), batches[0][1]
        assert r['noerr'] == c.kw['err_thr'] + (1 if above else 0) and r['noerr'] >= 3
        assert t[1] == ('pass' if above else 'repaired -1') or (not above and t[1] == 'repaired +1'), t
        assert t[0] in DEVICE and t[2] in DEVICE, t
    c.reach = reach
    return c


def lut_limits(mode):
    """The limits of the LDS copies: a bit LUT of 256 rows (symbol 255 valid, 256 irregular); an NRZ-S LUT of 2048 entries whose
    only match is in the last successor slot."""
    if mode == 'lut':
        lut = np.random.RandomState(7).randint(0, 2, 256).astype(np.uint8)
        lut[255] = 1
        plants = [{}, {100: 255, 101: 255}, {100: 256}, {}, {}]
    else:
        lut, plants = nrzs_lut_last_slot(), [{}] * 5
    c = Case(f'lut_limits-{mode}', 200, None, None, lut=lut)
    a = aft(mode, 40)
    specs = [sp(190, 25, a, slip=(b == 1), plant=plants[b]) for b in range(5)]
    c.steps = [('seed', NONE, NONE, None), ('batch', c.blocks(np.random.RandomState(8), specs))]

    def reach(batches):
        t, res = tags(batches), batches[0]
        if mode == 'lut':
            assert t[0] in DEVICE and t[1] in DEVICE and t[2] == t[3] == 'irregular' and t[4] in DEVICE and res[2]['host_error'], t
        else:
            assert all(x in DEVICE for x in t) and 'repaired +1' in t and 'repaired -1' in t, t
            assert all(r['noerr'] == 0 and 0 < r['bits'].sum() < r['nwin'] for r in res)
    c.reach = reach
    return c


def batch_sizes(mode, nb):
    """Batches of 1, 2, 63 and 64 blocks (cum[65]): three chained on the device's own carry, then one whose LAST block is irregular
    -- the next batch's block 0 is the host's (the carry is unknown), the blocks behind it are the device's."""
    lut = the_lut(mode)
    c = Case(f'batch_sizes-{mode}-{nb}', 128, None, None, lut=lut)
    a = aft(mode, 25)
    specs = [sp(120 - (b % 2), 24, a, slip=int(b % 7 == 3), plant={60: lut.shape[0]} if b == 4 * nb - 1 else None) for b in range(5 * nb)]
    blocks = c.blocks(np.random.RandomState(nb + 64 * (mode == 'nrzs')), specs)
    c.steps = [('seed', NONE, NONE, None)] + [('batch', blocks[i * nb:(i + 1) * nb]) for i in range(5)]

    def reach(batches):
        assert all(len(res) == nb for res in batches)
        assert all(x in DEVICE for x in tags(batches[:3])), tags(batches[:3])
        assert batches[3][-1]['tag'] == 'irregular' and batches[4][0]['tag'] == 'irregular' and batches[4][0]['ok']
        assert all(r['tag'] in DEVICE for r in batches[4][1:])
        if nb > 1:
            assert 'repaired +1' in tags(batches) and 'repaired -1' in tags(batches)
    c.reach = reach
    return c


# ---- A14 (bit LUT) ---------------------------------------------------------------------------------------------------------------
def _window_specs(nblocks, slips=()):
    return [sp(296, 23, 23, slip=int(b in slips)) for b in range(nblocks)]          # windows of 250 bits


def _template(rs, T, c):
    if T == 1:
        return np.ones(1, np.int8), 1
    t = (2 * rs.randint(0, 2, T) - 1).astype(np.int8)
    if T >= 3:
        t[T // 2] = 0                        # a tap of 0 belongs to neither mask
    if T >= 40:
        t[[0, T - 1, 31, 32]] = [1, -1, 0, 1]
    # bits are 0 / 1: a score has mean sum(t) / 2 and variance (taps != 0) / 4 on a random stream; c deviations above the mean
    return t, int(np.ceil(t.sum() / 2 + c * np.sqrt(np.count_nonzero(t)) / 2))


def _sync_reach(c, extra=None):
    def reach(batches):
        res = [r for b in batches for r in b]
        assert all(r['sync_valid'] == 1 and r['tag'] in DEVICE for r in res), tags(batches)
        for k in range(2):
            assert sum(len(r['hits'][k][0]) for r in res) > 0, k
        if extra:
            extra(res)
    c.reach = reach
    return c


TAP_BORDERS = [(1, 1), (1, 256), (31, 32), (32, 33), (255, 256), (256, 1), (64, 64)]


def tap_borders(T0, T1):
    """Tap counts on the word borders of the packed search."""
    rs = np.random.RandomState(1000 * T0 + T1)
    (t0, h0), (t1, h1) = _template(rs, T0, 2.2), _template(rs, T1, 2.0)
    c = Case(f'tap_borders-{T0}-{T1}', 300, None, None, templates=(t0, t1), thresholds=(h0, h1), nOv=300)
    b = c.blocks(rs, _window_specs(6, slips=(4,)))
    c.steps = [('seed', NONE, NONE, rs.randint(0, 2, 300).astype(np.uint8)), ('batch', b[:3]), ('batch', b[3:])]
    return _sync_reach(c)


REACH_BACK = [2048, 4096, 1, 38]


def reach_back(nOv):
    """Windows of 250 bits under a numBitsOverlap of 2048 / 4096: a block's stream spans eight / sixteen blocks and the ring
    (stream_at's walk back); numBitsOverlap of 1 and of T0 - 2 (the C ABI's contract, not enableStreamStages' narrower one)."""
    rs = np.random.RandomState(nOv)
    (t0, h0), (t1, h1) = _template(rs, 40, 2.6), _template(rs, 12, 2.8)
    nb = {2048: 10, 4096: 18}.get(nOv, 4)
    c = Case(f'reach_back-{nOv}', 300, None, None, templates=(t0, t1), thresholds=(h0, h1), nOv=nOv)
    b = c.blocks(rs, _window_specs(2 * nb, slips=(3,)))
    c.steps = [('seed', NONE, NONE, rs.randint(0, 2, nOv).astype(np.uint8)), ('batch', b[:nb]), ('batch', b[nb:])]

    def extra(res):
        if nOv >= 2048:
            assert sum(r['nwin'] for r in res[1:nb - 1]) < nOv - 40        # the last block of a batch reaches over all of them into the ring
            assert any(e['valid'] for r in res for e in r['edges'])
    return _sync_reach(c, extra)


def saturation_all():
    """All-(+1) templates with threshold 0: every position hits, the count is outLen, the first 64 are kept, every edge is invalid."""
    c = Case('saturation_all', 300, None, None, templates=(np.ones(16, np.int8), np.ones(12, np.int8)), thresholds=(0, 0), nOv=64)
    rs = np.random.RandomState(51)
    c.steps = [('seed', NONE, NONE, rs.randint(0, 2, 64).astype(np.uint8)), ('batch', c.blocks(rs, _window_specs(3)))]

    def extra(res):
        for r in res:
            assert [len(r['hits'][k][0]) for k in range(2)] == [64 + r['nwin'] + 15, 64 + r['nwin'] + 11]
            assert len(r['edges']) == 4 and not any(e['valid'] for e in r['edges'])
        assert all(e['ok'] and e['n'] == [15, 11] for r in res[1:] for e in r['edges'])
    return _sync_reach(c, extra)


def saturation_ones():
    """A one-tap template with threshold 1 on windows holding exactly 64 and exactly 65 ones (STREAM_MAX_HITS)."""
    c = Case('saturation_ones', 300, None, None, templates=(np.ones(1, np.int8), np.array([1, -1], np.int8)), thresholds=(1, 1), nOv=32)
    rs = np.random.RandomState(52)
    c.steps = []
    for ones in (64, 65):
        where = set((23 + rs.permutation(250)[:ones]).tolist())
        plant = {x: (1 if x in where else 0) for x in range(23, 273)}                  # LUT8: symbol 1 is a one, symbol 0 a zero
        c.steps += [('seed', NONE, NONE, np.zeros(32, np.uint8)), ('batch', c.blocks(rs, [sp(296, 23, 23, plant=plant)]))]

    def reach(batches):
        assert [len(res[0]['hits'][0][0]) for res in batches] == [64, 65]
        assert all(res[0]['sync_valid'] and res[0]['nwin'] == 250 for res in batches)
    c.reach = reach
    return c


def saturation_headers():
    """At least five header hits in a block (STREAM_EDGE_CANDS = 4), edges with at most 8 hits (valid) and with more (invalid)."""
    rs = np.random.RandomState(53)
    t0, t1 = (2 * rs.randint(0, 2, 24) - 1).astype(np.int8), (2 * rs.randint(0, 2, 64) - 1).astype(np.int8)
    c = Case('saturation_headers', 300, None, None, templates=(t0, t1), thresholds=(4, 4), nOv=300)
    b = c.blocks(rs, _window_specs(8))
    c.steps = [('seed', NONE, NONE, rs.randint(0, 2, 300).astype(np.uint8)), ('batch', b[:4]), ('batch', b[4:])]

    def extra(res):
        assert all(len(r['hits'][0][0]) >= 5 for r in res)
        E = [e for r in res for e in r['edges']]
        assert any(e['valid'] and 1 <= max(e['n']) <= 8 for e in E) and any(e['ok'] and max(e['n']) > 8 for e in E), [e['n'] for e in E]
        assert any(not e['ok'] for e in E)
    return _sync_reach(c, extra)


def ends(nOv):
    """A hit at position 0 and at outLen - 1 of both templates; outLen below 1024 (nOv 300) and at 2048 / 2049 (nOv 1800, 12 / 13
    taps): one position per thread, two, and the step to three."""
    def edge_template(T):
        t = -np.ones(T, np.int8)
        t[0] = t[-1] = 1
        return t
    c = Case(f'ends-{nOv}', 300, None, None, templates=(edge_template(12), edge_template(13)), thresholds=(1, 1), nOv=nOv)
    rs = np.random.RandomState(60 + nOv)
    ring = rs.randint(0, 2, nOv).astype(np.uint8)
    ring[0] = 1
    c.steps = [('seed', NONE, NONE, ring), ('batch', c.blocks(rs, [sp(283, 23, 23, plant={259: 1})]))]

    def reach(batches):
        r = batches[0][0]
        assert r['nwin'] == 237 and r['sync_valid']
        for k, T in enumerate((12, 13)):
            idx, outLen = r['hits'][k][0], nOv + 237 + T - 1
            assert outLen == {300: 548 + k, 1800: 2048 + k}[nOv]
            assert idx[0] == 0 and idx[-1] == outLen - 1 and len(idx) <= MAX_HITS, (k, idx)
    c.reach = reach
    return c


def validity():
    """sync_valid: an irregular block at index 2 of a batch (valid below it, not from it on), the next batch invalid until it is
    seeded again, a seed whose ring has the wrong length."""
    rs = np.random.RandomState(70)
    (t0, h0), (t1, h1) = _template(rs, 24, 2.0), _template(rs, 16, 2.0)
    c = Case('validity', 300, None, None, templates=(t0, t1), thresholds=(h0, h1), nOv=300)
    specs = _window_specs(20)
    specs[2]['plant'] = {100: 8}
    b = c.blocks(rs, specs)
    c.steps = [('seed', NONE, NONE, np.zeros(300, np.uint8)), ('batch', b[:5]), ('batch', b[5:10]), ('reseed',), ('batch', b[10:15]),
               ('seed', NONE, NONE, np.zeros(299, np.uint8)), ('batch', b[15:])]

    def reach(batches):
        v = [[r['sync_valid'] for r in res] for res in batches]
        assert v == [[1, 1, 0, 0, 0], [0] * 5, [1] * 5, [0] * 5], v
        assert tags(batches)[2:4] == ['irregular'] * 2 and all(x in DEVICE for x in tags(batches)[4:]), tags(batches)
        assert sum(len(r['hits'][0][0]) for r in batches[2]) > 0
    c.reach = reach
    return c


MODES = ('lut', 'nrzs')
CASES = {}
for _m in MODES:
    for _cap in (8192, 16384):
        CASES[f'second_stride-{_m}-{_cap}'] = functools.partial(second_stride, _m, _cap)
    CASES[f'count_tails-{_m}'] = functools.partial(count_tails, _m)
    CASES[f'tiny-{_m}'] = functools.partial(tiny, _m)
    for _o in (1, 2, 20, 30, 31):
        CASES[f'offset_limits-{_m}-{_o}'] = functools.partial(offset_limits, _m, _o)
    CASES[f'tails_batch-{_m}'] = functools.partial(tails_batch, _m)
    CASES[f'lut_limits-{_m}'] = functools.partial(lut_limits, _m)
    for _nb in (1, 2, 63, 64):
        CASES[f'batch_sizes-{_m}-{_nb}'] = functools.partial(batch_sizes, _m, _nb)
CASES['tails_seed'] = tails_seed
CASES['tails_noerr-equal'] = functools.partial(tails_noerr, False)
CASES['tails_noerr-above'] = functools.partial(tails_noerr, True)
for _t in TAP_BORDERS:
    CASES['tap_borders-%d-%d' % _t] = functools.partial(tap_borders, *_t)
for _n in REACH_BACK:
    CASES[f'reach_back-{_n}'] = functools.partial(reach_back, _n)
for _f in (saturation_all, saturation_ones, saturation_headers, validity):
    CASES[_f.__name__] = _f
for _n in (300, 1800):
    CASES[f'ends-{_n}'] = functools.partial(ends, _n)
# the cases the byte forms (k_stream_sync / k_stream_ring / k_stream_edges) run in their child process
BYTE_CASES = ['tap_borders-%d-%d' % t for t in TAP_BORDERS] + [f'reach_back-{n}' for n in REACH_BACK] + ['saturation_headers']


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once per process; nothing changes its blocks afterwards."""
    c = CASES[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def model_results(name):
    return drive(case(name))[0]


# ---- running a case --------------------------------------------------------------------------------------------------------------
SCALARS = ('a13_status', 'a13_start', 'a13_nwin', 'a13_npost', 'a13_nend', 'a13_noerr', 'sync_valid', 'sync_count')


def records(R):
    """What the tests look at of a BatchRecord, as arrays of their own."""
    rec = {k: np.asarray(R.s[k]) for k in SCALARS}
    rec.update(bits=R.bits.copy(), cen8=R.cen8.copy(), trust=R.trust.copy(), post=R.post.copy(), end=R.end.copy(), hits=R.hits.copy(),
               edges=R.edges.copy())
    return rec


def drive(c, bank=None):
    """(model results, device records) per 'batch' step; the device runs only when a bank is given."""
    m = StreamModel(**c.kw)
    if bank is not None:
        k = c.kw
        lut = {'bit_lut': k['lut']} if np.asarray(k['lut']).ndim == 1 else {'nrzs_lut': k['lut']}
        bank.set_stream_stages(k['overlap_samples'], k['o'], k['match_thr'], k['err_thr'], templates=k['templates'],
                               thresholds=k['thresholds'], bits_overlap=k['nOv'], **lut)
    results, recs = [], []
    for step in c.steps:
        if step[0] == 'batch':
            blocks = step[1]
            results.append(m.batch(blocks))
            if bank is not None:
                recs.append(records(bank.debug_stream_stages([g[0] for g in blocks], np.stack([g[1] for g in blocks]),
                                                             np.stack([g[2] for g in blocks]), np.stack([g[3] for g in blocks]))))
            continue
        post, end, ring = m.host_state() if step[0] == 'reseed' else step[1:]
        m.seed(post, end, ring)
        if bank is not None:
            bank.stream_seed(post, end, ring)
    return results, recs


def check_batch(results, rec, where):
    """One batch's device records against the model: the status of every block; for the blocks the device kept, everything."""
    for i, r in enumerate(results):
        at = (where, i, r['tag'])
        assert rec['a13_status'][i] == r['status'], (at, rec['a13_status'][i])
        assert rec['sync_valid'][i] == r['sync_valid'], at
        if r['status'] == 0:
            continue
        for k in ('nwin', 'start', 'npost', 'nend', 'noerr'):
            assert rec['a13_' + k][i] == r[k], (at, k, rec['a13_' + k][i], r[k])
        nw = r['nwin']
        for k in ('bits', 'cen8', 'trust'):
            assert np.array_equal(rec[k][i, :nw], r[k]), (at, k)
        assert np.array_equal(rec['post'][i, :r['npost']], r['post']) and np.array_equal(rec['end'][i, :r['nend']], r['end']), at
        if not r['sync_valid']:
            assert list(rec['sync_count'][i]) == [0, 0], at
            continue
        for k, (idx, score) in enumerate(r['hits']):
            n = rec['sync_count'][i][k]
            assert n == len(idx), (at, k, n, len(idx))
            n = min(n, MAX_HITS)                             # (a count beyond what the record holds is reported, the first 64 kept)
            assert np.array_equal(rec['hits'][i, k, 0, :n], idx[:n]) and np.array_equal(rec['hits'][i, k, 1, :n], score[:n]), (at, k)
        E, eh = rec['edges'][i], (rec['edges'].shape[2] - 4) // 4
        for ci in range(EDGE_CANDS):
            if ci >= len(r['edges']):
                assert E[ci, 1] == 0, (at, ci)
                continue
            e = r['edges'][ci]
            assert E[ci, 0] == e['a_rel'] and E[ci, 1] == int(e['valid']), (at, ci, E[ci, :4], e)
            if e['ok']:
                assert list(E[ci, 2:4]) == e['n'], (at, ci, E[ci, :4], e)
            if e['valid']:
                for k in range(2):
                    n = e['n'][k]
                    assert np.array_equal(E[ci, 4 + k * eh:4 + k * eh + n], e['idx'][k]), (at, ci, k)
                    assert np.array_equal(E[ci, 4 + 2 * eh + k * eh:4 + 2 * eh + k * eh + n], e['score'][k]), (at, ci, k)
