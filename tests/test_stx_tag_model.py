"""The numpy model of the device's clipped-peak tag (tests/stx_tag_model.py, k_stream_tag) against the host's own tagging in
Demodulator.demodulateHost (reference DB:830-837; the method itself runs, numpy's slicing included) on seeded draws, and the placements of the
GPU test's edge stream against the clip model (tests/clip_model.py, chained as the receive loop clips)."""
import numpy as np
import pytest

import stx_tag_model as tm


def _draw(rng, N, s, kind):
    """(centres of the kept window, ascending clip indices) of one draw."""
    sp = s - rng.uniform(0, 0.999) if s > 1 else 1.0          # ceil(spSym) == s
    nk = int(rng.integers(1, min(4000, max(2, N // max(1, int(sp))))))
    c = np.sort(rng.integers(0, N, nk)).astype(np.int32)
    if kind == 'edges':
        # peaks just below, at and above 2 s, near the end, and centres at every distance up to 2 s + 2 from them
        P = {max(0, 2 * s - 2), 2 * s - 1, 2 * s, 2 * s + 1, N - 1, max(0, N - 1 - 2 * s), int(rng.integers(0, 2 * s))}
        P |= set(rng.integers(0, N, 5).tolist())
        P = np.array(sorted(p for p in P if 0 <= p < N), np.int64)
        extra = (P[:, None] + np.arange(-2 * s - 2, 2 * s + 3)[None, :]).ravel()
        c = np.concatenate((c, extra[(extra >= 0) & (extra < N)].astype(np.int32)))
    elif kind == 'dense':
        p0 = int(rng.integers(0, N - 1))
        run = np.arange(p0, min(N, p0 + int(rng.integers(1, 3000))))
        P = np.unique(np.concatenate((run, rng.integers(0, N, int(rng.integers(0, 50))))))
    else:
        P = np.unique(rng.integers(0, N, int(rng.integers(0, 200))))
    if rng.uniform() < 0.2:
        c = np.concatenate((c, -rng.integers(1, N + 1, 5).astype(np.int32)))     # negative centres: marks[c + N]
    return sp, c, P.astype(np.int64)


@pytest.mark.parametrize('log2N', [12, 13, 15, 17, 20])
@pytest.mark.parametrize('kind', ['random', 'edges', 'dense'])
def test_model_equals_the_host_loop(log2N, kind):
    N = 1 << log2N
    rng = np.random.default_rng(log2N * 7 + len(kind))
    for trial in range(12 if log2N < 20 else 4):
        s = int(rng.integers(1, 129)) if trial else 128
        sp, c, P = _draw(rng, N, s, kind)
        assert int(np.ceil(sp)) == s
        trust = rng.integers(0, 256, len(c)).astype(np.uint8)
        assert np.array_equal(tm.tag(trust, c, P, sp, N), tm.host_tag(trust, c, P, sp, N)), (N, s, trial)


@pytest.mark.parametrize('N,s', [(4096, 1024), (4096, 1100), (4096, 3000), (8192, 2500), (4096, 4096)])
def test_negative_start_branch_tags_when_4s_plus_1_exceeds_N(N, s):
    """A peak below 2 s marks marks[p - 2 s + N : p + 2 s + 1]: empty unless 4 s + 1 > N; here it is not, and the model agrees."""
    assert 4 * s + 1 > N
    rng = np.random.default_rng(N + s)
    c = np.arange(N, dtype=np.int32)
    P = np.array(sorted({0, 3, min(2 * s - 1, N - 1), int(rng.integers(0, N))}), np.int64)
    trust = np.zeros(N, np.uint8)
    want = tm.host_tag(trust, c, P, float(s), N)
    assert np.array_equal(tm.tag(trust, c, P, float(s), N), want)
    only_small = P[P < 2 * s][:1]
    lo, hi = tm.tag_bounds(int(only_small[0]), s, N)
    assert hi > lo and (tm.host_tag(trust, c, only_small, float(s), N) == 254).sum() == hi - lo


def test_peak_below_2s_tags_nothing_at_2_17():
    N, s = 1 << 17, 20
    c = np.arange(N, dtype=np.int32)
    trust = np.zeros(N, np.uint8)
    for p in (0, 3, 2 * s - 1):
        assert not (tm.host_tag(trust, c, [p], s - 0.5, N) == 254).any()
        assert not (tm.tag(trust, c, [p], s - 0.5, N) == 254).any()
    for p in (2 * s, N - 1):
        lo, hi = tm.tag_bounds(p, s, N)
        assert np.array_equal(np.flatnonzero(tm.tag(trust, c, [p], s - 0.5, N) == 254), np.arange(lo, hi))


@pytest.mark.parametrize('mod', ['GMSK', 'BPSK'])
@pytest.mark.parametrize('bs', [15, 17])
def test_edge_stream_produces_its_clip_classes(mod, bs):
    N, ov, nblocks = 1 << bs, 1 << 11, tm.EDGE_BLOCKS
    full = tm.make_stream(mod, N, ov, nblocks, tm.edge_bursts(N, ov, nblocks), seed=5)
    idxs = tm.clip_chain(full, N, ov, nblocks, 4.5)
    classes = tm.edge_classes(idxs, N, ov, sps=16)
    # every class in the stream, and inside each batch of 4 / 16 blocks the GPU test's device runs finish (from block 2 B on)
    for first in (0, 8, 32):
        for c in tm.EDGE_CLASSES:
            assert any(c in k for k in classes[first:]), (first, c, classes)
        # a clip-free block between clipped ones
        assert any(not len(idxs[k]) and len(idxs[k - 1]) and len(idxs[k + 1]) for k in range(first + 1, nblocks - 1)), first
