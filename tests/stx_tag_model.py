"""numpy model of the clipped-peak tag of the S-band back end on the device (k_stream_tag, pycusdr_amd/csrc/stream_kernels.hpp):
the reference's trust tagging next to clipped interference peaks (demodulator_base.py:751-757, reference DB:830-837)

    marks = zeros(N, bool); s = int(ceil(spSym))
    for p in clipped: marks[p - 2 s : p + 2 s + 1] = 1
    trustSymbolWin[marks[centresWin]] = -2

restated per kept centre c with numpy's slice bounds: hi(p) = min(p + 2 s + 1, N); lo(p) = p - 2 s when that is >= 0, else
max(p - 2 s + N, 0) (a negative start counts from the end).  c is marked iff some p has lo(p) <= c < hi(p); for the ascending
indices P that is one binary search per branch:
    p >= 2 s:  the first p >= max(c - 2 s, 2 s) is <= c + 2 s
    p <  2 s:  the first p >= max(c - 2 s, 0)   is <= min(c + 2 s - N, 2 s - 1)
A centre in [-N, 0) indexes marks[c + N], as numpy does.

Also the seeded streams of tests/test_gpu_stx_stages.py: dense random bursts, and placements that put clipped peaks where the
tag has its edges."""
import numpy as np


def host_tag(trust_win, centres_win, clipped, spSym, N):
    """The host's own tagging: Demodulator.demodulateHost (demodulator_base.py) run on a block whose kept window is given --
    its bit lookup and alignment stand-ins hand back `centres_win` and the int8 trust bytes as checkSymbolOverlap would, and
    the method's own loop then tags them.  Returns its uint8 trust bytes."""
    import types
    from pycusdr_amd.demodulator.demodulator_base import Demodulator
    cw = np.asarray(centres_win, dtype=np.int32)
    tw = np.asarray(trust_win).view(np.int8).copy()
    stub = types.SimpleNamespace(
        Nfft=N, _rec_clips=Demodulator._rec_clips,
        hostBits=lambda rec: (np.zeros(len(cw), np.uint8), 0),
        checkSymbolOverlap=lambda noError, centres, idxSymbol, dataBits, trustSymbol: (cw, dataBits, tw, None))
    rec = {'spSym': spSym, 'symbols': np.zeros(len(cw), np.int32), 'centres': cw, 'trust': tw,
           'clipped': np.asarray(clipped, dtype=np.int64)}
    return Demodulator.demodulateHost(stub, rec)[2]


def tag_bounds(p, s, N):
    """[lo(p), hi(p)) of marks[p - 2 s : p + 2 s + 1] (numpy's slice, step 1)."""
    lo = p - 2 * s
    if lo < 0:
        lo = max(lo + N, 0)
    return lo, min(p + 2 * s + 1, N)


def tag_mask(centres_win, clipped, spSym, N):
    """Which kept symbols get the tag: the two binary searches of k_stream_tag, vectorised (int64 throughout)."""
    P = np.asarray(clipped, dtype=np.int64)
    c = np.asarray(centres_win, dtype=np.int64)
    c = np.where(c < 0, c + N, c)
    if not len(P) or not len(c):
        return np.zeros(len(c), dtype=bool)
    s2 = 2 * int(np.ceil(spSym))
    n = len(P)
    Pp = np.append(P, np.iinfo(np.int64).max)
    q = np.searchsorted(P, np.maximum(c - s2, s2), side='left')
    hit = Pp[q] <= c + s2
    top = np.minimum(c + s2 - N, s2 - 1)
    q2 = np.searchsorted(P, np.maximum(c - s2, 0), side='left')
    hit |= (top >= 0) & (q2 < n) & (Pp[q2] <= top)
    return hit


def tag(trust_win, centres_win, clipped, spSym, N):
    """The device's trust bytes (uint8) after the tag."""
    t = np.asarray(trust_win).view(np.uint8).copy()
    t[tag_mask(centres_win, clipped, spSym, N)] = 254
    return t


# ---- the streams of tests/test_gpu_stx_stages.py ---------------------------------------------------------------------------
EDGE_CLASSES = ('below_2s', 'first_half_overlap', 'last_half_overlap', 'near_end', 'long', 'clip_free')
# the edge stream's length: a receive loop's first block goes through the host code (there is no previous block to align
# against), and so do the batches begun before that is known -- with 16 blocks per call the third batch, blocks 32 ... 47, is
# the first the device finishes, all in one launch of the tag
EDGE_BLOCKS = 48


def edge_bursts(N, ov, nblocks, sps=16, seed=5):
    """Strong short bursts placed where the tag has its edges, in a stream of `nblocks` blocks (block k = samples
    [k (N - ov), k (N - ov) + N)), by block k mod 6:
        0  a burst of N/20 samples at 60 x: >= 1000 clipped samples, and a threshold well above block k + 1's
        1  peaks below 2 sps (3 ... 2 sps - 12, 2 sps - 1, 2 sps) and one inside the first half-overlap -- all inside the
           overlap block k - 1 clipped already: they are clipped again here because block k - 1's threshold was the higher one
        2  a peak inside the last half-overlap (N - ov/4) and one within 2 sps of the block's last sample (N - 6)
        3, 5  a burst in the middle
        4  nothing: a clip-free block between clipped ones
    Returns [(start, length, factor)]."""
    rng = np.random.default_rng(seed)
    stride = N - ov
    out = []
    for k in range(nblocks):
        b0, c = k * stride, k % 6
        if c == 0:
            out.append((b0 + N // 3, N // 20, 60.0))
        elif c == 1:
            out += [(b0 + int(rng.integers(3, 2 * sps - 12)), 1, 900.0), (b0 + 2 * sps - 1, 1, 900.0), (b0 + 2 * sps, 1, 900.0),
                    (b0 + ov // 4 + int(rng.integers(0, 64)), 3, 700.0)]
        elif c == 2:
            out += [(b0 + N - ov // 4 - int(rng.integers(0, 64)), 3, 700.0), (b0 + N - 6, 1, 900.0)]
        elif c in (3, 5):
            out.append((b0 + N // 2 + int(rng.integers(-N // 8, N // 8)), int(rng.integers(5, 40)), float(rng.uniform(50, 400))))
    return out


def burst_bursts(N, ov, nblocks, seed):
    """The dense random stream: per block two bursts inside its kept window (their tags reach kept symbols), one inside its
    last `ov` samples and one just after its start."""
    rng = np.random.default_rng(seed)
    stride = N - ov
    out = []
    for k in range(nblocks):
        b0 = k * stride
        for _ in range(2):
            out.append((b0 + int(rng.integers(ov, N - ov)), int(rng.integers(1, 40)), float(rng.uniform(50, 400))))
        out += [(b0 + N - ov + int(rng.integers(0, ov - 60)), 30, float(rng.uniform(50, 400))),
                (b0 + ov + int(rng.integers(0, 64)), 12, float(rng.uniform(50, 400)))]
    return out


def make_stream(mod, N, ov, nblocks, bursts, seed):
    """The samples a receive loop sees (its first block's overlap is zero): block k = full[k (N - ov) : k (N - ov) + N]."""
    from pycusdr_amd import signals as sg
    full = sg.s1_stream(nblocks, N, ov, mod, snr_db=12.0, seed=seed)[:nblocks * (N - ov) + ov].copy()
    full[:ov] = 0
    for p0, ln, f in bursts:
        full[p0:p0 + ln] *= np.float32(f)
    return full


def clip_chain(full, N, ov, nblocks, scale):
    """clippedPeakIPure of every block as the receive loop clips them (the overlap after clipping, reference DP:293,337)."""
    import clip_model as cm
    stride = N - ov
    carry, idxs = None, []
    for k in range(nblocks):
        x = full[k * stride:k * stride + N].copy()
        if carry is not None:
            x[:ov] = carry
        idxs.append(cm.clip(x, scale))
        carry = x[N - ov:].copy()
    return idxs


def edge_classes(idxs, N, ov, sps=16):
    """Per block: the set of EDGE_CLASSES its clip indices fall in."""
    s2 = 2 * sps
    out = []
    for P in idxs:
        P = np.asarray(P)
        c = set()
        if not len(P):
            c.add('clip_free')
        if (P < s2).any():
            c.add('below_2s')
        if ((P >= 0) & (P < ov // 2)).any():
            c.add('first_half_overlap')
        if ((P >= N - ov // 2) & (P < N)).any():
            c.add('last_half_overlap')
        if (P >= N - 1 - s2).any():
            c.add('near_end')
        if len(P) >= 1000:
            c.add('long')
        out.append(c)
    return out
