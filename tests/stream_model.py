"""What the stream-stage kernels (csrc/stream_kernels.hpp) promise, at any geometry, restated with the host code they replace:
``Demodulator.extractBits`` / ``extractBitsNRZs`` / ``checkSymbolOverlap`` on a plain namespace (as tests/test_demod_hostlogic.py
calls them), the uint8 casts of ``demodulateHost``, ``np.convolve`` on ring ++ bitsWin for the decoder's searches, the first T - 1
positions of the stream a stashed candidate would start for the edges, the last nOv bits for the ring.  Host only.

Per block the model says what the host code did, as a tag:
    device-expected   regular block, window not moved           (a13_status 1)
    repaired +1 / -1  regular block, the +-1 repair moved it     (a13_status 1)
    pass              too many impossible transitions: no alignment attempted  (a13_status 1)
    raised            the alignment's first comparison has operands of unequal length: nothing is adjusted  (a13_status 2)
    irregular         the host code raised IndexError / ValueError, or a precondition of the device path does not hold: the
                      block is the host's (a13_status 0)
The preconditions are the ones stream_kernels.hpp states in its head: every symbol index inside the LUT, a first and a last centre,
a window of at least o + 2 symbols that ends inside the decoded bits, a known predecessor, and -- where the comparison is made --
a previous tail of at least o + 1 bits behind and exactly o + 1 bits inside its window, o + 1 bits in front of this window, and a
tail that fits the record (512 bits)."""
import logging
import types

import numpy as np

from pycusdr_amd.demodulator import demodulator_base as dbm
from pycusdr_amd.demodulator.demodulator_base import Demodulator

POST_MAX, END_MAX, MAX_HITS, EDGE_CANDS, EDGE_HITS, EDGE_BACK = 512, 32, 64, 4, 8, 20
STATUS = {'irregular': 0, 'device-expected': 1, 'repaired +1': 1, 'repaired -1': 1, 'pass': 1, 'raised': 2}


class _Count(logging.Handler):
    def __init__(self):
        super().__init__()
        self.n = 0

    def emit(self, record):
        self.n += 1


def _first(mask):
    i = int(np.argmax(mask)) if len(mask) else 0
    return i if len(mask) and mask[i] else None


class StreamModel:
    def __init__(self, N, overlap_samples, o, match_thr, err_thr, lut, templates=(), thresholds=(), nOv=0):
        lut = np.asarray(lut)
        self.mode = 'lut' if lut.ndim == 1 else 'nrzs'
        self.N, self.ovw, self.o, self.err_thr = int(N), int(overlap_samples) // 2, int(o), int(err_thr)
        self.rows = lut.shape[0]
        self.host = types.SimpleNamespace(sigOverlapWin=self.ovw, Nfft=self.N, overlapOffset=self.o, symbol_check_match_threshold=match_thr,
                                          symbol_check_error_threshold=err_thr, poswinP=[], posSymEnd=[],
                                          bitLUT=lut.astype(np.uint8) if self.mode == 'lut' else None,
                                          symbolLUT=None if self.mode == 'lut' else lut.astype(np.int64))
        self.host.extractBitsNRZs = types.MethodType(Demodulator.extractBitsNRZs, self.host)
        self.templates = [np.asarray(t, dtype=np.int64) for t in templates]
        self.thresholds = [int(np.ceil(h)) for h in thresholds]
        self.nOv = int(nOv)
        self.known = False                       # does the device know the tail in front of the next batch?
        self.ring, self.ring_valid = np.zeros(self.nOv, np.int64), False         # the host's last nOv bits; does the device hold them?

    # -- what MFBank.stream_seed hands the device -------------------------------------------------------------------------------
    def seed(self, post, end, ring=None):
        self.host.poswinP, self.host.posSymEnd = np.asarray(post, dtype=np.uint8), np.asarray(end, dtype=np.uint8)
        self.known = True
        self.ring_valid = ring is not None and len(ring) == self.nOv and self.nOv > 0
        if self.ring_valid:
            self.ring = np.asarray(ring, dtype=np.int64)

    def host_state(self):
        """(post, end, ring) of the host code now: what a caller seeds the device with after a block went to the host."""
        return (np.asarray(self.host.poswinP, dtype=np.uint8), np.asarray(self.host.posSymEnd, dtype=np.uint8),
                self.ring.astype(np.uint8))

    # -- A12 + A13 of one block ---------------------------------------------------------------------------------------------------
    def _align(self, blk, known):
        count, sym, cen, mag = blk
        o, h = self.o, self.host
        s, c = np.asarray(sym[:count], dtype=np.int64), np.asarray(cen[:count], dtype=np.int64)
        trust = np.asarray(mag, dtype=np.float32).view(np.int8)[:count].copy()          # quirk Q3: the leading bytes of the magnitudes
        nbits = count if self.mode == 'lut' else count - 1
        start0, end0 = _first(c >= self.ovw), _first(c > self.N - self.ovw)
        ok = (bool(np.all((s >= 0) & (s < self.rows))) and start0 is not None and end0 is not None and end0 - start0 >= o + 2
              and end0 <= nbits and nbits > 0)
        prev_post, prev_end = h.poswinP, h.posSymEnd
        r = {'ok': ok, 'host_error': None, 'host_logged': False, 'count': count, 'start0': start0, 'end0': end0,
             'prev_npost': len(prev_post)}
        counter = _Count()
        dbm.log.addHandler(counter)
        try:
            bits, errs = Demodulator.extractBits(h, c, s)
            noerr = len(errs)
            cw, bw, tw, _ = Demodulator.checkSymbolOverlap(h, noerr, c, s, bits, trust)
        except (IndexError, ValueError) as e:            # what the reference does with such a block: the exception leaves the method
            r['host_error'] = str(e)
        finally:
            dbm.log.removeHandler(counter)
        r['host_logged'] = counter.n > 0
        if r['host_error'] is None:
            r.update(noerr=noerr, bits=np.asarray(bw).astype(np.uint8), cen8=np.asarray(cw).astype(np.uint8),
                     trust=np.asarray(tw).astype(np.uint8), post=np.asarray(h.poswinP).astype(np.uint8),
                     end=np.asarray(h.posSymEnd).astype(np.uint8))
            r['nwin'] = len(r['bits'])
        if r['host_error'] is not None or not ok or not known:
            tag = 'irregular'
        elif noerr > self.err_thr:
            tag = 'pass'
        elif 0 < len(prev_post) < o:                     # prev_post[:o] == win[:o] with unequal operands (the window has >= o + 2 bits)
            tag = 'raised'
        elif len(prev_post) > 0 and (len(prev_post) < o + 1 or len(prev_end) != o + 1 or start0 < o + 1 or count - end0 > POST_MAX):
            tag = 'irregular'
        else:
            tag = {0: 'device-expected', 1: 'repaired +1', -1: 'repaired -1'}[(end0 - r['nwin']) - start0]
        if tag != 'irregular' and nbits - end0 > POST_MAX:
            tag = 'irregular'
        if tag != 'irregular':
            r.update(start=end0 - r['nwin'], npost=nbits - end0, nend=o + 1)
            assert r['npost'] == len(r['post']) and len(r['end']) == o + 1
        r['tag'], r['status'] = tag, STATUS[tag]
        return r

    # -- A14 of one block: hits on ring ++ bitsWin, the would-be stash edges -----------------------------------------------------
    def _search(self, r, V, cum):
        """V: ring ++ the kept bits of the batch's blocks up to and including this one; cum: kept bits in front of it."""
        stream = V[cum:]
        L = len(stream)
        assert L == self.nOv + r['nwin']
        scores = [np.convolve(stream, t) for t in self.templates]
        r['hits'] = []
        for sc, thr in zip(scores, self.thresholds):
            idx = np.where(sc >= thr)[0]
            r['hits'].append((idx, sc[idx]))
        r['edges'] = []
        if len(self.templates) != 2:
            return
        Tm = max(len(t) for t in self.templates)
        for hdr in r['hits'][0][0][:min(EDGE_CANDS, MAX_HITS)]:
            a_rel = int(hdr) - len(self.templates[0]) + 1 - EDGE_BACK
            e = {'a_rel': a_rel, 'ok': cum + a_rel >= 0 and a_rel + Tm - 1 <= L, 'n': [0, 0], 'idx': [[], []], 'score': [[], []]}
            if e['ok']:
                lead = V[cum + a_rel:cum + a_rel + Tm - 1]          # the first Tmax - 1 bits of the stream a stash would start
                for k, (t, thr) in enumerate(zip(self.templates, self.thresholds)):
                    if len(t) > 1:
                        sc = np.convolve(lead, t)[:len(t) - 1]
                        idx = np.where(sc >= thr)[0]
                        e['n'][k], e['idx'][k], e['score'][k] = len(idx), idx, sc[idx]
            e['valid'] = bool(e['ok'] and max(e['n']) <= EDGE_HITS)
            r['edges'].append(e)

    def batch(self, blocks):
        """One device call on `blocks` = [(count, sym, cen, mag), ...]: one result dict per block; the state moves on as the host's
        and the device's do (the carry is unknown behind a last block that went to the host, the ring behind any)."""
        out, known = [], self.known
        V, cum, chain = self.ring.copy(), 0, self.ring_valid
        for blk in blocks:
            r = self._align(blk, known)
            known = r['ok']                      # the tail is a function of that block's symbols alone
            chain = chain and r['status'] != 0
            r['sync_valid'] = int(bool(chain and self.templates))
            if r['host_error'] is None:
                V = np.concatenate((V, r['bits'].astype(np.int64)))
                if r['sync_valid']:
                    self._search(r, V, cum)
                cum += r['nwin']
            out.append(r)
        self.known = out[-1]['status'] != 0
        self.ring_valid = bool(chain)
        self.ring = V[len(V) - self.nOv:]
        return out


# ---- blocks of one symbol stream with every constant an argument and the centres injected ----------------------------------------
def make_blocks(rs, lut, specs, N, overlap_samples, cap, p_err=0.0):
    """Symbol decisions of consecutive blocks of one stream.  ``specs``: one dict per block --
        count   symbols decided (<= cap, the record's capacity)
        start   centres below ov/2 (= the index of the window's first symbol)
        after   centres above N - ov/2 (the bits behind the window; NRZ-S: one more than bits)
        slip    block b shows global symbol S_b + x + slip at position x (a symbol-clock slip at the block edge)
        plant   {position: symbol index, or a function of the decisions so far} written over the decisions, in order
    The window of block b + 1 continues the stream where the window of block b ends.  Entries past `count` hold what must not be
    read as decisions: a symbol outside the LUT and a centre beyond the block."""
    lut = np.asarray(lut)
    mode = 'lut' if lut.ndim == 1 else 'nrzs'
    rows, ovw = lut.shape[0], overlap_samples // 2
    bases, E = [], max(sp['start'] for sp in specs) + 4
    for sp in specs:
        bases.append(E - sp['start'])
        E += max(sp['count'] - sp['after'] - sp['start'], 0)
    total = max(b + sp['count'] for b, sp in zip(bases, specs)) + 8
    if mode == 'lut':
        gbits = rs.randint(0, 2, total)
        classes = [np.where(lut == v)[0] for v in (0, 1)]
    else:                             # NRZ-S: a random walk through the LUT's successor sets (entries outside the LUT are no successors)
        cand = [[[int(v) for v in lut[s, k] if 0 <= v < rows] or [s] for k in (0, 1)] for s in range(rows)]
        rb, rq = rs.randint(0, 2, total).tolist(), rs.randint(0, 1 << 30, total).tolist()
        g = [int(rs.randint(0, rows))] * total
        for i in range(1, total):
            c = cand[g[i - 1]][rb[i]]
            g[i] = c[rq[i] % len(c)]
        g = np.asarray(g, dtype=np.int64)
    out = []
    for base, sp in zip(bases, specs):
        count, start, after = sp['count'], sp['start'], sp['after']
        mid = max(count - start - after, 0)
        cen = np.full(cap, N, dtype=np.int32)
        parts = [np.linspace(0, ovw - 1, start), np.linspace(ovw, N - ovw, mid), np.linspace(N - ovw + 1, N - 1, after)]
        cen[:count] = np.concatenate(parts).astype(np.int32)[:count]
        idx = np.clip(base + np.arange(count) + sp.get('slip', 0), 0, total - 1)
        sym = np.full(cap, rows + 7, dtype=np.int32)
        if mode == 'lut':
            bits = gbits[idx] ^ (rs.rand(count) < p_err)
            pick = rs.randint(0, 1 << 30, count)
            sym[:count] = np.where(bits != 0, classes[1][pick % len(classes[1])], classes[0][pick % len(classes[0])])
        else:
            sym[:count] = g[idx]
        for x, v in sp.get('plant', {}).items():
            sym[x] = v(sym) if callable(v) else v
        mag = rs.randint(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32).view(np.float32)
        out.append((count, sym, cen, mag))
    return out
