"""The modulator's kernels (pycusdr_amd/csrc/mod_kernels.hpp) through the C ABI, against the integer model of
tests/modulator_model.py: phase words bit for bit (mfb_debug_mod_phase), samples within 4 * 2^-24 per component of the float64
value of their word, pads bit for bit.

What decides the shapes: k_mod_rows runs one thread per bit of the whole batch in workgroups of 256, so a frame boundary may
fall anywhere in a wave or workgroup; k_mod_scan runs one workgroup of 256 per frame and walks the frame in tiles of 1024
symbols (four waves of 64 lanes, four consecutive symbols per lane), so a frame's own length decides its lane, wave and tile
edges: 2 and 3 sit inside one lane, 255 / 256 / 257 at the wave edge, 1023 / 1025 at the tile edge; k_mod_samples runs one thread
per output sample in workgroups of 256 and finds the frame once per workgroup where the workgroup lies inside one frame, by
bisection per thread where a frame boundary falls inside it (frames of 2 x 2 samples put dozens of frames into one)."""
import ctypes as C

import numpy as np
import pytest

import modulator_model as mm

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025]
KINDS = {'FSK': mm.FSK, 'GMSK': mm.GMSK3}


def lut_of(mod, sps):
    from pycusdr_amd.modulator import modulators
    cls = modulators.FSKmod if mod == 'FSK' else modulators.GMSKmod
    return cls(None, {'samplesPerSym': sps}).LUT


@pytest.fixture(scope='module')
def dev():
    from pycusdr_amd.modulator.device import DeviceModulator
    d = DeviceModulator(1 << 15, 1 << 20)
    yield d
    d.close()


def run(dev, frames, dphi, words=True):
    dev.begin(frames, dphi)
    sig, off = dev.end()
    return sig, off, (dev.phase_words() if words else None)


def check_batch(dev, mod, lut, frames, dphi, noise=None, pad=0, min_len=0):
    """One device call against the model, frame by frame.  Returns the worst component error seen."""
    sps = lut.shape[1]
    sig, off, words = run(dev, frames, dphi)
    assert sig.dtype == np.complex64 and len(sig) == off[-1] == len(words)
    worst = 0.0
    for f, bits in enumerate(frames):
        n = len(bits) * sps
        pre, total = mm.layout(n, pad, min_len)
        assert off[f + 1] - off[f] == total, (f, len(bits))
        s, w = sig[off[f]:off[f + 1]], words[off[f]:off[f + 1]]
        want = mm.words(KINDS[mod], lut, bits, 0.0 if dphi is None else dphi[f])
        body = slice(pre + pad, pre + pad + n)
        bad = np.flatnonzero(w[body] != want)
        assert bad.size == 0, (mod, sps, f, len(bits), bad[:4], w[body][bad[:4]], want[bad[:4]])
        err = mm.component_error(s[body], want)
        assert err <= mm.BOUND, (mod, sps, f, len(bits), err / 2.0 ** -24)
        worst = max(worst, err)
        if pad or pre:
            assert s[:pre].tobytes() == noise[:pre].tobytes(), f
            assert s[pre:pre + pad].tobytes() == noise[:pad].tobytes(), f
            assert s[pre + pad + n:].tobytes() == noise[:pad].tobytes(), f
            assert not w[:pre + pad].any() and not w[pre + pad + n:].any()
    return worst


@pytest.mark.parametrize('sps', [2, 5, 16, 128])
@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_phase_words_and_samples(dev, mod, sps):
    """Every frame length around the wave and tile edges of the scan, as one batch, without and with a frame increment."""
    rs = np.random.RandomState(100 + sps)
    lut = lut_of(mod, sps)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(None, 0, 0)
    lengths = ([1] if mod == 'FSK' else []) + LENGTHS
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in lengths]
    worst = check_batch(dev, mod, lut, frames, None)
    dphi = rs.uniform(-3.0, 3.0, len(frames))
    dphi[0] = 1e6          # far outside one turn
    worst = max(worst, check_batch(dev, mod, lut, frames, dphi))
    print(f'{mod} spSym {sps}: worst component error {worst / 2.0 ** -24:.3f} * 2^-24')


@pytest.mark.parametrize('mod', ['FSK', 'GMSK'])
def test_batch_of_nine_with_boundaries_at_wave_and_tile_edges(dev, mod):
    """Frame boundaries at bits 64, 127, 193, 256, 511, 769, 1024, 1026: on, just before and just after a wave (64) and a
    workgroup / tile (256) edge of the row kernel's grid.  All-ones frames beside all-zeros frames: a GMSK edge rule that read
    the neighbour frame's bit would change the first or last row.  Pads and the short-frame pre-pad on."""
    rs = np.random.RandomState(7)
    lut = lut_of(mod, 5)
    noise = (rs.randn(700) + 1j * rs.randn(700)).astype(np.complex64)
    dev.set_lut(KINDS[mod], lut)
    dev.set_pad(noise, 7, 600)
    lengths = [64, 63, 66, 63, 255, 258, 255, 2, 300]
    assert list(np.cumsum(lengths)[:8]) == [64, 127, 193, 256, 511, 769, 1024, 1026]
    frames = [np.full(n, (i + 1) % 2, np.uint8) for i, n in enumerate(lengths)]
    frames[4] = rs.randint(0, 2, 255).astype(np.uint8)
    frames[8] = rs.randint(0, 2, 300).astype(np.uint8)
    dphi = rs.uniform(-1.0, 1.0, 9)
    check_batch(dev, mod, lut, frames, dphi, noise, 7, 600)
    assert mm.layout(64 * 5, 7, 600)[0] == 600 - 334 and mm.layout(255 * 5, 7, 600)[0] == 0      # both kinds of frame were in it
    dev.set_pad(None, 0, 0)


def test_one_long_frame_walks_many_tiles(dev):
    """5000 bits: five tiles of 1024 symbols with the running sum carried, the last one partial."""
    rs = np.random.RandomState(8)
    for mod in ('FSK', 'GMSK'):
        lut = lut_of(mod, 5)
        dev.set_lut(KINDS[mod], lut)
        check_batch(dev, mod, lut, [rs.randint(0, 2, 5000).astype(np.uint8)], np.array([0.777]))


def test_same_bytes_twice_and_frame_by_frame(dev):
    rs = np.random.RandomState(9)
    lut = lut_of('GMSK', 16)
    noise = (rs.randn(64) + 1j * rs.randn(64)).astype(np.complex64)
    dev.set_lut(mm.GMSK3, lut)
    dev.set_pad(noise, 33, 0)
    frames = [rs.randint(0, 2, n).astype(np.uint8) for n in (65, 2, 257, 300, 64)]
    dphi = rs.uniform(-1.0, 1.0, len(frames))
    a, off, wa = run(dev, frames, dphi)
    b, off2, wb = run(dev, frames, dphi)
    assert a.tobytes() == b.tobytes() and wa.tobytes() == wb.tobytes() and np.array_equal(off, off2)
    for f, bits in enumerate(frames):
        one, o1, w1 = run(dev, [bits], dphi[f:f + 1])
        assert one.tobytes() == a[off[f]:off[f + 1]].tobytes() and w1.tobytes() == wa[off[f]:off[f + 1]].tobytes(), f
    # left on the device (no copy in mfb_modulator_end): the same words, and the page-locked view holds the same bytes
    dev.begin(frames, dphi)
    batch = dev.end(copy=False)
    assert batch.ptr and batch.total == len(a) and batch.frame_ptr(1) == batch.ptr + 8 * off[1] and batch.frame_len(1) == off[2] - off[1]
    assert dev.phase_words().tobytes() == wa.tobytes()
    dev.begin(frames, dphi)
    pinned, _ = dev.end(pinned=True)
    assert pinned.tobytes() == a.tobytes()
    dev.set_pad(None, 0, 0)


def test_misuse_returns_codes_and_the_handle_still_works():
    from pycusdr_amd import _lib
    lib = _lib.load()
    OK, ARG, STATE, UNSUP = _lib.MFB_OK, _lib.MFB_ERR_ARG, _lib.MFB_ERR_STATE, _lib.MFB_ERR_UNSUPPORTED
    h = C.c_void_p()
    assert lib.mfb_modulator_create(C.byref(h), 0, 0, 1024) == ARG and not h
    assert lib.mfb_modulator_create(C.byref(h), 0, 1 << 23, 1024) == UNSUP
    assert lib.mfb_modulator_create(C.byref(h), 0, 1024, (1 << 24) + 1) == UNSUP
    assert lib.mfb_modulator_create(C.byref(h), 0, 1024, 4096) == OK
    try:
        bits = np.array([1, 0, 1, 1, 0], np.uint8)
        off = np.array([0, 5], np.int32)
        out = np.zeros(2 * 4096, np.float32)
        soff = np.zeros(2, np.int64)

        def begin(b=bits, o=off, d=None, B=1):
            return lib.mfb_modulator_begin(h, b.ctypes.data, o.ctypes.data, d, B)

        assert begin() == STATE                                                   # no LUT set
        assert lib.mfb_modulator_end(h, out.ctypes.data, soff.ctypes.data) == STATE      # end without begin
        ptr, n = C.c_void_p(), C.c_int64()
        assert lib.mfb_modulator_device_output(h, C.byref(ptr), C.byref(n)) == STATE
        assert lib.mfb_debug_mod_phase(h, out.ctypes.data, 4096) == STATE
        g = np.ascontiguousarray(lut_of('GMSK', 16))
        assert lib.mfb_modulator_set_lut(h, mm.GMSK3, g.ctypes.data, 2, 16) == ARG       # GMSK has eight rows
        assert lib.mfb_modulator_set_lut(h, 7, g.ctypes.data, 8, 16) == ARG
        assert lib.mfb_modulator_set_lut(h, mm.GMSK3, g.ctypes.data, 8, 1) == UNSUP
        assert lib.mfb_modulator_set_lut(h, mm.GMSK3, g.ctypes.data, 8, 1025) == UNSUP
        assert begin() == STATE                                                   # still none
        assert lib.mfb_modulator_set_lut(h, mm.GMSK3, g.ctypes.data, 8, 16) == OK
        assert begin(o=np.array([0, 1], np.int32)) == ARG                         # GMSK with < 2 bits
        assert begin(o=np.array([0, 0], np.int32)) == ARG                         # a frame of 0 bits
        assert begin(o=np.array([0, 3, 3], np.int32), B=2) == ARG                 # ... inside a batch
        assert begin(o=np.array([1, 5], np.int32)) == ARG
        assert begin(B=0) == ARG
        assert begin(b=np.zeros(2000, np.uint8), o=np.array([0, 2000], np.int32)) == ARG      # more bits than created for
        assert begin(b=np.zeros(1000, np.uint8), o=np.array([0, 1000], np.int32)) == ARG      # 16 000 samples > 4096
        assert lib.mfb_modulator_begin(h, None, off.ctypes.data, None, 1) == ARG
        assert lib.mfb_modulator_set_pad(h, None, 0, 4, 0) == ARG
        noise = np.zeros(8, np.complex64)
        assert lib.mfb_modulator_set_pad(h, noise.ctypes.data, 8, 4, 9) == ARG    # min_len beyond the noise
        assert begin() == OK
        assert begin() == STATE                                                   # a call in flight
        assert lib.mfb_modulator_set_lut(h, mm.GMSK3, g.ctypes.data, 8, 16) == STATE
        assert lib.mfb_modulator_set_pad(h, None, 0, 0, 0) == STATE
        assert lib.mfb_modulator_device_output(h, C.byref(ptr), C.byref(n)) == STATE
        assert lib.mfb_modulator_end(h, out.ctypes.data, soff.ctypes.data) == OK
        assert lib.mfb_modulator_end(h, out.ctypes.data, soff.ctypes.data) == STATE
        assert list(soff) == [0, 80]
        words = np.zeros(80, np.uint64)
        assert lib.mfb_debug_mod_phase(h, words.ctypes.data, 79) == ARG
        assert lib.mfb_debug_mod_phase(h, words.ctypes.data, 80) == OK
        # after all that the handle computes what a fresh one would
        assert np.array_equal(words, mm.words(mm.GMSK3, g, bits))
        assert mm.component_error(out[:160].view(np.complex64), words) <= mm.BOUND
        f = np.ascontiguousarray(lut_of('FSK', 16))
        assert lib.mfb_modulator_set_lut(h, mm.FSK, f.ctypes.data, 2, 16) == OK
        assert lib.mfb_debug_mod_phase(h, words.ctypes.data, 80) == STATE         # the batch belonged to the old table
        assert begin(b=bits[:1], o=np.array([0, 1], np.int32)) == OK              # one bit is a frame for FSK
        assert lib.mfb_modulator_end(h, None, None) == OK
        assert lib.mfb_debug_mod_phase(h, words.ctypes.data, 80) == OK
        assert np.array_equal(words[:16], mm.words(mm.FSK, f, bits[:1]))
    finally:
        assert lib.mfb_modulator_destroy(h) == OK
    assert lib.mfb_modulator_destroy(None) == ARG
