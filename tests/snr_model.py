"""numpy model of the device's window means (pycusdr_amd/csrc/snr_kernels.hpp): ``np.mean(np.abs(window))`` of a complex64 window
made of one or two pieces, in the kernel's exact operation order, so that a device result can be compared bit for bit with what
``Demodulator.computeSNR`` (reference demodulator/demodulator_base.py:635-667) takes from the spectrum slices on the host.

  |x|    ``clip_model.npabs`` (numpy's complex absolute value)
  sum    8192-element chunks folded in order (s = chunk0; s = s + chunk1; ...); a chunk of n elements is numpy's pairwise sum:
         n < 8 a plain loop from 0; n <= 128 eight strided accumulators seeded with the first eight elements, advanced over
         n - n % 8 elements, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 remaining elements one by
         one; otherwise split at n2 = n / 2 - (n / 2) % 8 and add the two halves' sums
  mean   float32(float64(sum) / n); NaN for an empty window
The kernel lays the recursion of a chunk out as a binary heap of 255 slots (at most 7 splits) and adds the inner nodes level by level;
``chunk_sum`` does the same, so that the heap's depth bound is part of what the model checks.
"""
import numpy as np

from clip_model import npabs

f32 = np.float32
CHUNK, LEAF, DEPTH = 8192, 128, 7
NODES = (2 << DEPTH) - 1

# the window lengths the tests walk: every length up to 300, and the ones around a leaf tree's and a chunk's edges
LENGTHS = list(range(0, 301)) + [1023, 1024, 1025, 8191, 8192, 8193, 8199, 8200, 16389, 1 << 15]
# two pieces (as a band that wraps around 0 Hz): odd lengths on both sides of 128 and of 8192
PAIRS = [(1, 1), (3, 5), (7, 121), (121, 7), (63, 65), (65, 63), (127, 1), (1, 127), (127, 3), (129, 127), (5, 8187), (8187, 5), (4095, 4097),
         (8191, 1), (1, 8191), (8191, 3), (8193, 8191), (0, 9), (9, 0), (0, 0)]


def leaf_sum(v):
    n = len(v)
    with np.errstate(all='ignore'):
        if n < 8:
            s = f32(0)
            for x in v:
                s = f32(s + x)
            return s
        body = n - n % 8
        r = v[:8].copy()
        for i in range(8, body, 8):
            r = (r + v[i:i + 8]).astype(f32)
        s = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
        for x in v[body:]:
            s = f32(s + x)
        return s


def heap_nodes(m):
    """Per heap slot of a chunk of m elements: (offset, length) of a leaf, -1 for an inner node, None where there is no node."""
    nodes = [None] * NODES
    for h in range(NODES):
        d = (h + 1).bit_length() - 1
        k = h + 1 - (1 << d)
        off, ln = 0, m
        for lv in range(d - 1, -1, -1):
            if ln <= LEAF:
                ln = 0
                break
            n2 = ln // 2 - (ln // 2) % 8
            if (k >> lv) & 1:
                off, ln = off + n2, ln - n2
            else:
                ln = n2
        if ln > LEAF:
            assert d < DEPTH, 'the recursion is deeper than the heap'
            nodes[h] = -1
        elif ln > 0:
            nodes[h] = (off, ln)
    return nodes


def chunk_sum(v):
    nodes = heap_nodes(len(v))
    val = [None] * NODES
    for h, nd in enumerate(nodes):
        if nd is not None and nd != -1:
            val[h] = leaf_sum(v[nd[0]:nd[0] + nd[1]])
    with np.errstate(all='ignore'):
        for d in range(DEPTH - 1, -1, -1):
            for h in range((1 << d) - 1, (2 << d) - 1):
                if nodes[h] == -1:
                    val[h] = f32(val[2 * h + 1] + val[2 * h + 2])
    return val[0]


def window_mean(pieces):
    """float32 mean of |x| over the concatenation of ``pieces`` (one or two complex64 arrays), as the kernel computes it."""
    mag = np.concatenate([npabs(np.asarray(p, dtype=np.complex64)) for p in pieces]) if len(pieces) else np.zeros(0, f32)
    n = len(mag)
    if n == 0:
        return f32(np.nan)
    s = None
    with np.errstate(all='ignore'):
        for c in range(0, n, CHUNK):
            cs = chunk_sum(mag[c:c + CHUNK])
            s = cs if s is None else f32(s + cs)
        return f32(np.float64(s) / np.float64(n))


def spread(rng, n, zeros=True):
    """complex64 samples whose amplitudes spread over many decades (a wrong summation order changes the float32 sum), some exact
    zeros among them."""
    amp = 10.0 ** rng.uniform(-12, 12, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    x = (amp * np.exp(1j * ph)).astype(np.complex64)
    if zeros and n:
        x[rng.integers(0, n, max(1, n // 50))] = 0
    return x


def left_to_right(mag):
    """The plain float32 sum s = ((m0 + m1) + m2) + ... (cumsum adds in that order)."""
    with np.errstate(all='ignore'):
        return np.cumsum(mag, dtype=f32)[-1] if len(mag) else f32(0)


def sensitive(n, tag=0):
    """``spread`` samples, n of them, on which numpy's float32 sum of |x| differs from the plain left-to-right sum (n > 128: the
    first of the seeds (n, tag, 0), (n, tag, 1), ... that shows it) -- a model or a kernel that adds in another order than numpy's
    then gives other bits.  Up to 128 elements a few orders coincide too often to insist."""
    for attempt in range(64):
        x = spread(np.random.default_rng((n, tag, attempt)), n)
        mag = np.abs(x)
        if n <= LEAF or left_to_right(mag) != np.add.reduce(mag):
            return x
    raise AssertionError(f'no order-sensitive input of {n} elements')


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN matching any NaN (its sign and payload are the host's, not numpy's rule)."""
    a, b = np.atleast_1d(np.asarray(a, f32)), np.atleast_1d(np.asarray(b, f32))
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))
