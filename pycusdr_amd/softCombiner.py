"""Soft combiner: several receivers demodulate the same transmission; their bit streams are aligned by
cross-correlation, voted bit by bit with the trust bytes, and one stream per master goes on to the decoder.

Restates the deterministic part of the reference's softCombiner.py -- ``Worker`` (the index bookkeeping,
softCombiner.py:92-451), ``SoftCombiner.correlate`` (:665-798), ``_doVoteN`` (:570-618), ``_doVote2`` (:623-662) and
``compareWorkers`` (:807-838) -- as plain classes: no process, no sockets, no timer; the caller inserts worker data and
calls ``compareWorkers()``, which returns the dicts the reference would push to its decoder socket.  Out of scope: the
unused per-slave pairing (``Slave``, ``getSelf(slaveId)``) and ``removeData``.

Two back ends compute the core and give identical results:

* ``'host'``: numpy.  The alignment correlation is the reference's FFT form rounded to the integers it stands for.
* ``'hip'``:  ``mfbank.Combiner`` (csrc/combine_kernels.hpp): packed popcount correlation, top-15, decisions and the
  vote on the device, one round trip per master.  Every decision is re-checked on the host from the returned integer
  ``val[]`` with numpy's own mean / std; on a disagreement (a knife edge between the device's and numpy's float64
  rounding), with more than three slaves or streams beyond 2^20 bits the call is redone on the host path.

Deviation from the reference: a slave buffer of fewer than 16 bits is not evaluated and never matched.
"""
import logging
import time

import numpy as np

log = logging.getLogger('pycusdr_amd.' + __name__)

DATATYPE = np.int8
TRUSTTYPE = np.int8
MAX_DATA_LEN_BEFORE_TRANSMIT = 6000       # an unmatched master with more new bits than this is sent at once
NUM_PEAKS = 15
MIN_SLAVE_BITS = 16

NOTHING, COMBINED, MASTER_ONLY = 0, 1, 2

# what a disagreement of two voters is tagged with before the sign flip and the int8 cast (both make 0 of the fractions)
BOTH_TRUST_ERR, MASTER_TRUST, SLAVE_TRUST, BOTH_DISTRUST = 0.1, 0.7, 0.3, -1


class WorkerIdError(AssertionError):
    pass


def _to_int8(x):
    """float64 -> int8 as a C cast does it for values in range, and wrapping (not platform-defined) beyond."""
    return np.trunc(x).astype(np.int64).astype(np.int8)


# ---- the votes -------------------------------------------------------------------------------------------------------------
def vote2(bitsM, trustM, bitsS, trustS):
    """Master and one slave.  Agreeing bits pass with trust -1.  Where they disagree the master's bit wins unless the
    master distrusts its bit (trust < 0) and the slave trusts its own (trust > 0); the trust byte becomes +1 when both
    distrust, 0 otherwise."""
    bM, bS = np.asarray(bitsM), np.asarray(bitsS)
    tM, tS = np.asarray(trustM), np.asarray(trustS)
    total = bM + bS
    differ = total == 1
    bits = (total / 2).astype(DATATYPE)            # 0 where they differ: overwritten below unless nobody decides
    tag = np.ones(len(bM), dtype=TRUSTTYPE)
    s_neg, m_neg, s_pos = tS < 0, tM < 0, tS > 0
    use_master = differ & (s_neg | ~m_neg)
    use_slave = differ & ~s_neg & m_neg & s_pos
    bits[use_master] = bM[use_master]
    bits[use_slave] = bS[use_slave]
    tag[use_master | use_slave] = 0                # 0.7, 0.3 and 0.1 stored into int8
    tag[differ & s_neg & m_neg] = BOTH_DISTRUST
    return bits, -tag


def voteN(bitsM, trustM, bitsS, trustS, weight):
    """Master and two or more slaves.  Voters with trust < 0 abstain; the master's bit counts ``weight``; the bit is 1
    when the weighted sum exceeds half the (weighted) number of voters left.  The trust byte follows the reference's
    arithmetic literally (softCombiner.py:606-609), float steps and casts included."""
    rows = [np.asarray(bitsM).astype(float) * weight] + [np.asarray(b).astype(float) for b in bitsS]
    trust = [np.asarray(trustM)] + [np.asarray(t) for t in trustS]
    nv = len(rows)
    for r, t in zip(rows, trust):
        r[t < 0] = 0
    qualified = sum((t >= 0).astype(np.int64) for t in trust)
    threshold = qualified.astype(float) / 2
    threshold[trust[0] >= 0] += weight / 2
    total = rows[0].copy()
    for r in rows[1:]:
        total = total + r
    bits = (total > threshold).astype(DATATYPE)
    out = nv / 10 - sum((t == -1).astype(np.int64) for t in trust) / 10
    one, zero = total == 1, total == 0
    out[one] += _to_int8(total[one])
    base = out[zero] * 10 + nv
    acc = rows[0][zero] - base
    for r in rows[1:]:
        acc = acc + (r[zero] - base)
    out[zero] += _to_int8(acc)
    return bits, _to_int8(out)


TRUST_CLASS_REPRESENTATIVE = np.array([-2, -1, 0, 1], dtype=np.int8)     # classes {< -1, -1, 0, > 0}


def vote_table(voters, weight):
    """Output (bits uint8, trust int8) of the vote for every column state of ``voters`` voters: entry sum_v code_v 8^v,
    code_v = 4 bit_v + trust class, v = 0 the master.  Both votes look at one column at a time and at trust only
    through the four classes, so the table is the vote."""
    e = np.arange(8 ** voters)
    codes = [(e >> (3 * v)) & 7 for v in range(voters)]
    bits = [(c >> 2).astype(DATATYPE) for c in codes]
    trust = [TRUST_CLASS_REPRESENTATIVE[c & 3] for c in codes]
    if voters == 2:
        b, t = vote2(bits[0], trust[0], bits[1], trust[1])
    else:
        b, t = voteN(bits[0], trust[0], bits[1:], trust[1:], weight)
    return b.astype(np.uint8), t.astype(np.int8)


def column_states(bits, trust):
    """Table index of every column: ``bits`` / ``trust`` are lists over voters (master first) of equal-length arrays."""
    s = np.zeros(len(bits[0]), dtype=np.int64)
    for v, (b, t) in enumerate(zip(bits, trust)):
        t = np.asarray(t).astype(np.int64)
        cls = np.where(t < -1, 0, np.where(t == -1, 1, np.where(t == 0, 2, 3)))
        s |= ((np.asarray(b) != 0) * 4 + cls) << (3 * v)
    return s


# ---- the core on the host --------------------------------------------------------------------------------------------------
def pow2ceil(n):
    N = 1
    while N < n:
        N *= 2
    return N


def bit_xcorr_host(slave_bits, master_bits):
    """x[k] = sum_j bT[(j + k) mod N] bM[j] over the first min(len(master), n) master bits: the reference's
    abs(customXCorr(bitsX, bitsM[:n])) rounded to the integers it stands for (float64 FFT: the error is ~1e-10)."""
    a = np.asarray(slave_bits).astype(np.float64)
    n = len(a)
    N = pow2ceil(n)
    b = np.asarray(master_bits)[:n].astype(np.float64)
    x = np.fft.irfft(np.fft.rfft(a, N) * np.conj(np.fft.rfft(b, N)), N) if N > 1 else a[:1] * b[:1]
    return np.rint(x).astype(np.int64)


def top_peaks(x):
    """The fifteen largest values by repeated arg-max with zeroing (ties: lowest index) and the first one's index."""
    x = np.array(x, dtype=np.int64)
    val = np.zeros(NUM_PEAKS, dtype=np.int64)
    idx0 = 0
    for i in range(NUM_PEAKS):
        k = int(np.argmax(x))
        if i == 0:
            idx0 = k
        val[i] = x[k]
        x[k] = 0
    return val, idx0


def decision(val, variance_multiplier):
    """(cond, matched) from the fifteen peak values, in numpy's float64 as the reference computes it."""
    v = np.asarray(val, dtype=np.float64)
    cond = np.mean(v[2:]) + variance_multiplier * np.std(v[2:])
    return float(cond), bool(v[0] > cond)


def _blank_record():
    return {'evaluated': 0, 'matched': 0, 'idx0': 0, 'avail': 0, 'lc_after': 0, 'val': np.zeros(NUM_PEAKS, np.int32), 'cond': 0.0}


def combine_host(bitsM, trustM, slaves, variance_multiplier, weight, min_length, tables=None):
    """The core in numpy; the same dict as ``mfbank.Combiner.end``."""
    bitsM, trustM = np.asarray(bitsM), np.asarray(trustM)
    Lc = len(bitsM)
    recs, matched = [], []
    status = None
    for i, (bT, tT) in enumerate(slaves):
        n = len(bT)
        if status == NOTHING or n < MIN_SLAVE_BITS:
            recs.append(_blank_record())
            continue
        val, idx0 = top_peaks(bit_xcorr_host(bT, bitsM[:Lc]))
        cond, ok = decision(val, variance_multiplier)
        rec = {'evaluated': 1, 'matched': int(ok), 'idx0': idx0, 'avail': 0, 'lc_after': Lc, 'val': val.astype(np.int32), 'cond': cond}
        if ok:
            avail = max(0, min(Lc, n - idx0))
            rec['avail'] = avail
            if avail < min_length:
                status = NOTHING
            else:
                Lc = min(Lc, avail)
                matched.append(i)
                rec['lc_after'] = Lc
        recs.append(rec)
    if status == NOTHING:
        return {'status': NOTHING, 'bits': np.empty(0, np.uint8), 'trust': np.empty(0, np.int8), 'matched': [], 'slaves': recs}
    mb, mt = bitsM[:Lc], trustM[:Lc]
    if not matched:
        return {'status': MASTER_ONLY, 'bits': mb.astype(np.uint8), 'trust': mt.astype(np.int8), 'matched': [], 'slaves': recs}
    sb = [np.asarray(slaves[i][0])[recs[i]['idx0']:recs[i]['idx0'] + Lc] for i in matched]
    st = [np.asarray(slaves[i][1])[recs[i]['idx0']:recs[i]['idx0'] + Lc] for i in matched]
    if tables is not None:
        tb, tt = tables[len(matched) + 1]
        s = column_states([mb] + sb, [mt] + st)
        bits, trust = tb[s], tt[s]
    elif len(matched) == 1:
        bits, trust = vote2(mb, mt, sb[0], st[0])
    else:
        bits, trust = voteN(mb, mt, sb, st, weight)
    return {'status': COMBINED, 'bits': bits.astype(np.uint8), 'trust': trust.astype(np.int8), 'matched': matched, 'slaves': recs}


# ---- one worker's buffers ----------------------------------------------------------------------------------------------------
class Worker:
    """The bits and trust bytes one demodulator has delivered and not yet aged out, with the head / tail of what has
    been handed on.  ``clock`` replaces time.time (tests inject one)."""

    keyNames = ['count', 'timestamp', 'voteGroup', 'doppler', 'doppler_std', 'spSymEst', 'SNR', 'baudRate', 'protocol']
    keyDataTypes = {'count': int, 'timestamp': float, 'voteGroup': int, 'doppler': float, 'doppler_std': float, 'spSymEst': float,
                    'SNR': float, 'TxRangeRate': float, 'baudRate': int, 'protocol': str}
    arrayKeyNames = ['data', 'trust']
    arrayDataTypes = {'data': DATATYPE, 'trust': TRUSTTYPE}

    def __init__(self, workerData, timestampTimeOut=.5, showWarnings=False, clock=time.time):
        self.clock = clock
        self.showWarnings = showWarnings
        self.getCount = 0                  # blocks handed on (getSelf with new data), minus those handed back unused
        self.totalRequestCount = 0
        self._dataRequestCounter = 0       # requests since data of this worker was last sent on
        self.arrivalTimes = [{'time': clock(), 'idx': 0}]
        self.data = {}
        self.workerId = str(workerData['workerId'])
        self.timestamp = clock()
        for key in self.keyNames:
            self._add(key, workerData)
        for key in self.arrayKeyNames:
            self.data[key] = np.array([], dtype=self.arrayDataTypes[key])
            self._append(key, workerData)
        self.voteGroup = self.data.get('voteGroup', 0)
        assert len(self.data['data']) == len(self.data['trust']), 'data and trust have different lengths'
        self.head = 0
        self.tail = len(self.data['data'])
        self.timestampTimeOut = timestampTimeOut

    def _add(self, key, src):
        if key in src:
            try:
                self.data[key] = self.keyDataTypes[key](src[key])
            except Exception as e:          # noqa: BLE001 -- a malformed statistic is logged, the bits still count
                log.error('worker %s: cannot store %s: %s', self.workerId, key, e)
        elif self.showWarnings:
            log.warning('key %s not found for worker %s', key, src['workerId'])

    def _append(self, key, src):
        if key in src:
            self.data[key] = np.r_[self.data[key], np.array(src[key], dtype=self.arrayDataTypes[key])]
        elif self.showWarnings:
            log.warning('key %s not found for worker %s', key, src['workerId'])

    def clearDataRequestCounter(self):
        self._dataRequestCounter = 0

    def getDataRequestCounter(self):
        return self._dataRequestCounter

    def insertData(self, workerData):
        if not self.workerId == workerData['workerId']:
            raise WorkerIdError('Data workerId %s does not match worker workerId %s' % (workerData['workerId'], self.workerId))
        self.arrivalTimes.append({'time': self.clock(), 'idx': self.tail})
        if 'count' in self.data and workerData.get('count', 0) - 1 > self.data['count']:
            log.warning('worker %s: missing %d packets', self.workerId, workerData['count'] - self.data['count'] - 1)
        for key in self.keyNames:
            self._add(key, workerData)
        for key in self.arrayKeyNames:
            self._append(key, workerData)
        self.tail = len(self.data['data'])
        assert len(self.data['data']) == len(self.data['trust']), 'data and trust have different lengths'

    def getData(self, idx=None):
        if idx is None:
            return self.data['data'], self.data['trust']
        if idx >= len(self.data['data']):
            raise IndexError('Index out of range')
        return self.data['data'][:idx], self.data['trust'][:idx]

    def updateIdx(self, idx, dataUsed=True):
        """Hand ``idx`` bits back: they are offered again by the next getSelf."""
        self.head -= idx
        if not dataUsed:
            self.getCount -= 1

    def getSelf(self):
        """The statistics and the bits / trust not handed on yet, which then count as handed on."""
        out = {'workerId': self.workerId}
        for key in self.keyNames:
            out[key] = self.data.get(key, [])
        for key in self.arrayKeyNames:
            out[key] = self.data[key][self.head:self.tail]
        out['count'] = self.getCount
        if len(out['data']) > 0:
            self.totalRequestCount += 1
            self._dataRequestCounter += 1
            self.getCount += 1
        self.head = self.tail
        return out

    def removeOldData(self):
        """Drop the blocks that arrived more than timestampTimeOut ago; the newest block always stays."""
        while self.arrivalTimes[0]['time'] < self.clock() - self.timestampTimeOut and len(self.arrivalTimes) > 1:
            newHead = self.arrivalTimes[1]['idx']
            for key in self.arrayKeyNames:
                self.data[key] = self.data[key][newHead:]
            if self.head < newHead:
                log.warning('worker %s: removing more data than has been processed', self.workerId)
                self.head = 0
            else:
                self.head -= newHead
            self.tail -= newHead
            for at in self.arrivalTimes[1:]:
                at['idx'] -= newHead
            self.arrivalTimes.pop(0)

    def __eq__(self, other):
        return isinstance(other, self.__class__) and self.workerId == other.workerId and self.timestamp == other.timestamp

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None


# ---- the combiner ------------------------------------------------------------------------------------------------------------
class SoftCombiner:
    """``insert(workerData)`` files a demodulator's dict (workerId, count, data, trust, voteGroup, ...) under its worker;
    ``compareWorkers()`` takes every worker in turn as the master against all others and returns the combined dicts."""

    def __init__(self, conf, backend='hip', device=0, clock=time.time):
        if backend not in ('host', 'hip'):
            raise ValueError("backend is 'host' or 'hip'")
        sc = conf['SoftCombiner']
        self.conf = conf
        self.dataRequestThreshold = sc['workerDataRequestThreshold']
        self.MIN_LENGTH = sc['minProcessingLength']
        self.workerDataTimeout = sc['workerDataTimeout']
        self.varMultiplier = sc['varianceMultiplier']
        self.masterVoteWeight = sc['masterVoteWeight']
        self.pollingTimeout = sc.get('pollingTimeout')
        self.workerTimeout = sc.get('workerTimeout')
        self.compareInterval = sc.get('processingInterval')
        self.backend, self.device, self.clock = backend, device, clock
        self.workers = []
        self.tables = {v: vote_table(v, self.masterVoteWeight) for v in (2, 3, 4)}
        self.host_fallbacks = 0           # calls of the hip back end that were redone on the host path
        self._combiner = None

    def close(self):
        if self._combiner is not None:
            self._combiner.close()
            self._combiner = None

    def insert(self, workerData):
        workerId = workerData.get('workerId')
        if workerId is None:
            raise ValueError("worker data without 'workerId'")
        for w in self.workers:
            if w.workerId == str(workerId):
                w.insertData(workerData)
                return w
        w = Worker(workerData, timestampTimeOut=self.workerDataTimeout, clock=self.clock)
        self.workers.append(w)
        return w

    # the two back ends
    def _core_host(self, bitsM, trustM, slaves):
        return combine_host(bitsM, trustM, slaves, self.varMultiplier, self.masterVoteWeight, self.MIN_LENGTH)

    def _core_hip(self, bitsM, trustM, slaves):
        from . import mfbank
        longest = max([len(bitsM)] + [len(b) for b, _ in slaves])
        if len(slaves) > mfbank.COMBINE_MAX_SLAVES or longest > mfbank.COMBINE_MAX_BITS:
            self.host_fallbacks += 1
            return self._core_host(bitsM, trustM, slaves)
        if self._combiner is None:
            self._combiner = mfbank.Combiner(max_bits=max(1 << 16, longest), device=self.device)
            for v, (b, t) in self.tables.items():
                self._combiner.set_vote(v, b, t)
        res = self._combiner.combine(bitsM, trustM, slaves, self.varMultiplier, self.MIN_LENGTH)
        for r in res['slaves']:
            if r['evaluated'] and decision(r['val'], self.varMultiplier)[1] != bool(r['matched']):
                self.host_fallbacks += 1
                return self._core_host(bitsM, trustM, slaves)
        return res

    def combine(self, bitsM, trustM, slaves):
        """The core on this combiner's back end: master bits / trust and a list of (bits, trust) slave buffers."""
        return (self._core_hip if self.backend == 'hip' else self._core_host)(bitsM, trustM, slaves)

    def correlate(self, master, slaves):
        """One master against the slaves of its vote group; the dict for the decoder, or None when there is nothing new,
        a matched slave overlaps too little, or an unmatched master is held back for another cycle."""
        dataM = master.getSelf()
        if len(dataM['data']) == 0:
            return None
        bitsM, trustM = dataM['data'], dataM['trust']
        group = [s for s in slaves if s.voteGroup == master.voteGroup]
        res = self.combine(bitsM, trustM, [s.getData() for s in group])
        Lc = len(bitsM)
        for r in res['slaves']:                         # the master's head follows every truncation
            if not r['matched']:
                continue
            if r['avail'] < self.MIN_LENGTH:
                master.updateIdx(Lc, dataUsed=False)
                return None
            if r['avail'] < Lc:
                master.updateIdx(Lc - r['avail'])
                Lc = r['avail']
        names = [group[i].workerId for i in res['matched']]
        if res['status'] == COMBINED:
            dataM['data'] = res['bits'].view(DATATYPE)
            dataM['trust'] = res['trust']
        elif len(dataM['data']) <= MAX_DATA_LEN_BEFORE_TRANSMIT and master.getDataRequestCounter() < self.dataRequestThreshold:
            master.updateIdx(len(bitsM), dataUsed=False)        # wait another cycle for a slave to match
            return None
        master.clearDataRequestCounter()
        dataM['numSlaves'] = len(names)
        dataM['slaveNames'] = names
        return dataM

    def compareWorkers(self):
        out = []
        for m in range(len(self.workers)):
            slaves = self.workers.copy()
            master = slaves.pop(m)
            data = self.correlate(master, slaves)
            if data:
                out.append(data)
        for w in self.workers:
            w.removeOldData()
        return out
