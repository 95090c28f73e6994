"""The modulator's kernels (pycusdr_amd/csrc/mod_kernels.hpp) on the paths the whole-chain tests never take, through
``DeviceModulator`` with injected tables, against the integer model of tests/modulator_model.py.

The tables are arbitrary doubles, negative ones and ones beyond +-2 pi among them, so a row's total is an arbitrary 64-bit word
and every sum wraps.  Throughout: ``phase_words()`` equals ``mm.words`` bit for bit in the signal and is 0 in the pads, a sample
lies within ``mm.BOUND`` per component of ``mm.iq`` of its word, the pads are ``mm.frame``'s noise byte for byte, ``sample_off``
is ``mm.layout``'s.  tests/test_edge_shapes_host.py proves that the shapes of tests/edge_shapes.py reach what they are here for:
the two branches that correct k_mod_samples' symbol index, its bisection among many frames of one workgroup, k_mod_scan's tile,
thread and carry edges."""
import numpy as np
import pytest

import edge_shapes as es
import modulator_model as mm

pytestmark = pytest.mark.gpu

KINDS = {'FSK': mm.FSK, 'GMSK': mm.GMSK3}
ROWS = {'FSK': 2, 'GMSK': 8}


def lut_of(rs, mod, sps):
    lut = rs.uniform(-20.0, 20.0, (ROWS[mod], sps))
    lut[0, 0] = -4.0 * np.pi - 1.0e-9        # two turns back and a little: a word next to 2^64
    lut[-1, -1] = 7.0 * np.pi                # three and a half turns on
    assert lut.min() < -2 * np.pi and lut.max() > 2 * np.pi
    return lut


def noise_of(rs, n):
    return (rs.standard_normal(n) + 1j * rs.standard_normal(n)).astype(np.complex64)


@pytest.fixture(scope='module')
def dev():
    from pycusdr_amd.modulator.device import DeviceModulator
    d = DeviceModulator(1 << 18, 1 << 20)
    yield d
    d.close()


def check(dev, mod, lut, frames, dphi, noise=None, pad=0, min_len=0, packed=None):
    """One call against the model, frame by frame; returns (sample_off, worst component error).  ``packed``: the bytes to send
    instead of the frames' 0 / 1."""
    sps = lut.shape[1]
    if packed is None:
        dev.begin(frames, dphi)
    else:
        dev.begin_packed(*packed, dphi)
    sig, off = dev.end()
    words = dev.phase_words()
    assert sig.dtype == np.complex64 and len(sig) == off[-1] == len(words)
    want_off = np.concatenate(([0], np.cumsum([mm.layout(len(b) * sps, pad, min_len)[1] for b in frames])))
    assert np.array_equal(off, want_off)
    worst = 0.0
    for f, bits in enumerate(frames):
        n = len(bits) * sps
        pre, _ = mm.layout(n, pad, min_len)
        s, w = sig[off[f]:off[f + 1]], words[off[f]:off[f + 1]]
        want = mm.words(KINDS[mod], lut, bits, 0.0 if dphi is None else dphi[f])
        body = slice(pre + pad, pre + pad + n)
        bad = np.flatnonzero(w[body] != want)
        assert bad.size == 0, (mod, sps, f, len(bits), bad[:4], w[body][bad[:4]], want[bad[:4]])
        err = mm.component_error(s[body], want)
        assert err <= mm.BOUND, (mod, sps, f, len(bits), err / 2.0 ** -24)
        worst = max(worst, err)
        assert not w[:pre + pad].any() and not w[pre + pad + n:].any(), f
        if pad or pre:
            whole = mm.frame(np.zeros(n, np.complex64), noise, pad, min_len)
            assert len(whole) == len(s)
            assert s[:pre + pad].tobytes() == whole[:pre + pad].tobytes(), f
            assert s[pre + pad + n:].tobytes() == whole[pre + pad + n:].tobytes(), f
    return off, worst


@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_scan_tile_edges(dev, mod):
    """k_mod_scan: frames of 2 .. 2^17 symbols around the thread (4), wave (256), tile (1024) and multi-tile edges, the longest
    one 128 tiles with the carry running; increments of 0, a small step, a step that wraps at every symbol, half a turn."""
    rs = np.random.RandomState(21)
    lut = lut_of(rs, mod, es.SCAN_SPS)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(None, 0, 0)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in es.SCAN_LENGTHS]
    for rot in es.SCAN_ROTATIONS:
        dphi = np.array([es.SCAN_DPHI[(i + rot) % len(es.SCAN_DPHI)] for i in range(len(frames))])
        _, worst = check(dev, mod, lut, frames, dphi)
        print(f'{mod} scan edges, rotation {rot}: worst component error {worst / 2.0 ** -24:.3f} * 2^-24')


@pytest.mark.parametrize('sps', es.MANY_SPS)
@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_many_frames_in_one_workgroup(dev, mod, sps):
    """k_mod_samples: dozens of frames per 256-sample workgroup, so its third bisection chooses among many; boundaries on the
    last, first and second thread of a workgroup; a distinct increment per frame, so a wrong frame index changes the words."""
    rs = np.random.RandomState(22 + sps)
    min_bits = 1 if mod == 'FSK' else 2
    lengths, residues = es.many_frame_lengths(sps, min_bits, 11)
    lut = lut_of(rs, mod, sps)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(None, 0, 0)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in lengths]
    dphi = rs.uniform(-3.0, 3.0, len(frames))
    assert len(set(mm.quantise(dphi).tolist())) == len(frames)
    off, _ = check(dev, mod, lut, frames, dphi)
    hit = set((off[1:-1] % es.MOD_WORKGROUP).tolist())
    assert set(residues) <= hit, (residues, sorted(hit))
    if sps % 2:
        assert {255, 0, 1} <= hit
    per_group = np.bincount(off[1:-1] // es.MOD_WORKGROUP)
    assert per_group.max() >= 24


@pytest.mark.parametrize('pad,min_len', es.PADS)
@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_pads_that_are_not_tile_shaped(dev, mod, pad, min_len):
    """noise[0:pre], noise[0:pad], signal, noise[0:pad] with distinct random noise; short frames (pre > 0) and long ones (pre == 0)
    in one batch where there is a minimum length."""
    rs = np.random.RandomState(23)
    lut = lut_of(rs, mod, es.PAD_SPS)
    noise = noise_of(rs, 1000)
    assert len(set(noise.tolist())) == len(noise)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(noise, pad, min_len)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in es.PAD_BITS]
    pres = [mm.layout(len(b) * es.PAD_SPS, pad, min_len)[0] for b in frames]
    assert (min(pres) == 0 and max(pres) > 0) if min_len else max(pres) == 0
    check(dev, mod, lut, frames, rs.uniform(-1.0, 1.0, len(frames)), noise, pad, min_len)
    dev.set_pad(None, 0, 0)


@pytest.mark.parametrize('sps', es.MOD_UP_SPS)
@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_symbol_index_corrected_upward(dev, mod, sps):
    """k_mod_samples' `j >= sps`: the fp32 estimate of k / sps falls one short at these sps, first at k = sps."""
    rs = np.random.RandomState(24 + sps)
    lut = lut_of(rs, mod, sps)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(None, 0, 0)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in es.MOD_UP_BITS]
    check(dev, mod, lut, frames, rs.uniform(-1.0, 1.0, len(frames)))


def test_symbol_index_corrected_downward():
    """k_mod_samples' `j < 0`: one FSK frame of 33 300 bits at 255 samples per symbol, 8.49 M samples, in a handle created for
    exactly that.  All the words; the samples of the last 2^16, where the branch runs (k = 8 487 929)."""
    from pycusdr_amd.modulator.device import DeviceModulator
    sps, nbits = es.MOD_DOWN
    rs = np.random.RandomState(25)
    lut = lut_of(rs, 'FSK', sps)
    bits = rs.randint(0, 2, nbits).astype(np.uint8)
    d = DeviceModulator(nbits, nbits * sps)
    try:
        d.set_lut(mm.FSK, lut)
        d.begin([bits], np.array([0.4321]))
        sig, off = d.end()
        words = d.phase_words()
    finally:
        d.close()
    assert list(off) == [0, nbits * sps] and len(sig) == len(words) == nbits * sps
    want = mm.words(mm.FSK, lut, bits, 0.4321)
    bad = np.flatnonzero(words != want)
    assert bad.size == 0, (bad[:4], words[bad[:4]], want[bad[:4]])
    tail = slice(nbits * sps - (1 << 16), nbits * sps)
    err = mm.component_error(sig[tail], want[tail])
    assert err <= mm.BOUND, err / 2.0 ** -24


def test_gmsk_rows_at_frame_edges(dev):
    """All-ones frames beside all-zeros frames, in both orders: the bit beyond either end of a frame is 0, never the
    neighbour's.  (Also for FSK, whose rows have no neighbours: the batch is the same.)"""
    rs = np.random.RandomState(26)
    pattern = [(1, 5), (0, 5), (0, 4), (1, 3), (1, 2), (0, 2), (1, 6), (0, 3), (1, 2)]
    frames = [np.full(n, b, np.uint8) for b, n in pattern]
    edges = {(a[0], b[0]) for a, b in zip(pattern[:-1], pattern[1:])}
    assert edges == {(0, 0), (0, 1), (1, 0), (1, 1)}
    dev.set_pad(None, 0, 0)
    for mod in ('GMSK', 'FSK'):
        lut = lut_of(rs, mod, 3)
        # rows 4 b[s-1] + 2 b[s] + b[s+1]: all eight totals distinct, so a neighbour's bit changes the words
        assert len(set(mm.quantise(lut).sum(axis=1, dtype=np.uint64).tolist())) == ROWS[mod]
        dev.set_lut(KINDS[mod], lut)
        check(dev, mod, lut, frames, rs.uniform(-1.0, 1.0, len(frames)))


@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_bit_bytes_other_than_0_and_1(dev, mod):
    """Bytes 2, 0x80 and 255 are the bit 1, a frame's first byte among them (it sets the FSK initial word on the host)."""
    rs = np.random.RandomState(27)
    lut = lut_of(rs, mod, 5)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(None, 0, 0)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in (7, 2, 64, 300)]
    for f, b in enumerate(frames):
        b[0] = 1 if f != 1 else 0
        b[-1] = 1
    bits, off = dev.pack(frames)
    raw = bits.copy()
    ones = np.flatnonzero(bits)
    raw[ones] = np.array([2, 0x80, 255], np.uint8)[np.arange(len(ones)) % 3]
    assert set(raw.tolist()) == {0, 2, 0x80, 255} and all(raw[off[f]] > 1 for f in (0, 2, 3)) and raw[off[1]] == 0
    check(dev, mod, lut, frames, rs.uniform(-1.0, 1.0, len(frames)), packed=(raw, off))
