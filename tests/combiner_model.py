"""Plain references for the soft combiner's kernels (pycusdr_amd/csrc/combine_kernels.hpp), shared by test_combiner_model.py
(no GPU: the references against the definition and against numpy) and test_gpu_combiner_kernels.py (the kernels against them).
Nothing here uses floating point where the kernel claims integers, and nothing uses numpy where the kernel claims numpy's bits:

* ``exact_xcorr``    -- the circular correlation of the kernel's header comment in integer arithmetic, without an FFT;
* ``decision_exact`` -- ``cond`` in Python floats, one IEEE operation after the other in the order cmb_sum13 documents;
* ``decide_state``   -- what k_cmb_decide does with a decision: combine_host's bookkeeping (softCombiner.py) for one slave.
"""
import math

import numpy as np

NOTHING, COMBINED, MASTER_ONLY = 0, 1, 2
SLOT = 3            # bytes per slot of the big-integer product: a lag is at most 2^20 < 2^24, so no slot carries into the next


def pow2ceil(n):
    N = 1
    while N < n:
        N *= 2
    return N


def _spread(bits):
    """The integer sum_i bits[i] * 2^(24 i)."""
    buf = np.zeros((len(bits), SLOT), dtype=np.uint8)
    buf[:, 0] = bits
    return int.from_bytes(buf.tobytes(), 'little')


def exact_xcorr(slave_bits, master_bits):
    """x[k] = sum_{j < min(m, n)} a[(j + k) mod N] * b[j] for k in [0, N), N = 2^ceil(log2 n), a = the slave zero-padded to N: int64 [N].
    One product of two big integers gives every linear lag d = i - j in a slot of its own (the master reversed, so that slot
    d + L - 1 collects a[i] b[j]); the circular form adds the lags that are congruent modulo N."""
    a = (np.asarray(slave_bits) != 0).astype(np.uint8)
    n = len(a)
    N = pow2ceil(n)
    b = (np.asarray(master_bits)[:n] != 0).astype(np.uint8)
    L = len(b)
    assert n >= 1 and L >= 1 and min(n, L) < 1 << (8 * SLOT)
    nslots = n + L - 1
    prod = _spread(a) * _spread(b[::-1])
    raw = np.frombuffer(prod.to_bytes(SLOT * nslots, 'little'), dtype=np.uint8).reshape(nslots, SLOT).astype(np.int64)
    lin = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    x = np.zeros(N, dtype=np.int64)
    np.add.at(x, (np.arange(nslots) - (L - 1)) % N, lin)
    return x


def xcorr_by_definition(slave_bits, master_bits):
    """The same by the definition's loops: for the smallest shapes only."""
    a = [int(v != 0) for v in slave_bits]
    n = len(a)
    N = pow2ceil(n)
    a += [0] * (N - n)
    b = [int(v != 0) for v in master_bits][:n]
    return np.array([sum(a[(j + k) % N] * b[j] for j in range(len(b))) for k in range(N)], dtype=np.int64)


def _sum13(a):
    """numpy's float64 sum of 13 values: the pairwise routine below its block size -- eight partial sums, which for 13 values are
    the first eight values, combined as a tree, then the remaining five in order."""
    r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))
    for i in range(8, 13):
        r = r + a[i]
    return r


def decision_exact(val, variance_multiplier):
    """(cond, matched): cond = mean(val[2:]) + vm * std(val[2:]) of the fifteen peak values.  Python floats are IEEE doubles and
    every operation below is one correctly rounded operation (math.sqrt is; ``** 0.5`` is not), so this is the value the kernel
    claims: numpy's, bit for bit."""
    v = [float(int(t)) for t in val]
    assert len(v) == 15
    mean = _sum13(v[2:]) / 13.0
    dev = [t - mean for t in v[2:]]
    sd = math.sqrt(_sum13([t * t for t in dev]) / 13.0)
    cond = mean + float(variance_multiplier) * sd
    return cond, v[0] > cond


def decide_state(val, idx0, n, Lc, min_length, variance_multiplier):
    """One slave's bookkeeping after its peaks: a dict of matched, avail, lc_after (the master's length after this slave) and
    status -- NOTHING when a matched slave holds fewer than min_length bits from idx0 on, else COMBINED / MASTER_ONLY as a call
    of this one slave would end."""
    cond, ok = decision_exact(val, variance_multiplier)
    out = {'matched': int(ok), 'avail': 0, 'lc_after': int(Lc), 'status': MASTER_ONLY, 'cond': cond}
    if ok:
        avail = max(0, min(int(Lc), int(n) - int(idx0)))
        out['avail'] = avail
        if avail < min_length:
            out['status'] = NOTHING
        else:
            out['lc_after'] = min(int(Lc), avail)
            out['status'] = COMBINED
    return out
