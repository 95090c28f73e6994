"""The transmit side on the host: tables, framer, the integer phase and the 'host' back end of Modulator against fixtures
recorded from the reference (tests/golden/make_golden_modulator.py) and against the yardstick model (modulator_model.py)."""
import math
import os
import re

import numpy as np
import pytest

import modulator_model as mm
from pycusdr_amd import config as cfg
from pycusdr_amd.modulator import DataLengthError, Modulator, modulators, phase
from pycusdr_amd.protocol import loadProtocol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {'FSK': mm.FSK, 'GMSK': mm.GMSK3}


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_goldens_modulator.npz'), allow_pickle=False)
    return {k.replace('__', '/'): z[k] for k in z.files}


def radio_of(gold, sps):
    fc, fo, baud, cfo, _ = gold['radio']
    return {'frequency_Hz': float(fc), 'frequencyOffset_Hz': float(fo), 'baud': float(baud), 'centreFrequencyOffset': float(cfo),
            'samplesPerSym': sps}


def make_modulator(gold, mod, sps, backend, noise=None):
    """A Modulator on the fixture's radio: CC11xx for FSK, the GMSK bench protocol for GMSK."""
    if mod == 'FSK':
        proto = loadProtocol('CC11xx')(conf=cfg.cc11xx_config(samplesPerSym=sps))
    else:
        proto = loadProtocol('bench_GMSK')(conf=cfg.bench_config('bench_GMSK'))
    m = Modulator({}, radio_of(gold, sps), proto, backend=backend, noise=gold['noise'] if noise is None else noise)
    m.set_rangerate(float(gold['radio'][4]))
    return m


def comp_dist(a, b):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return max(np.abs(a.real - b.real).max(), np.abs(a.imag - b.imag).max())


def test_luts_equal_the_reference_bit_for_bit(gold):
    for sps in (2, 5, 16, 128):
        for mod, cls in (('FSK', modulators.FSKmod), ('GMSK', modulators.GMSKmod)):
            lut = cls(None, {'samplesPerSym': sps}).LUT
            ref = gold[f'lut/{mod}/{sps}']
            assert lut.dtype == np.float64 and lut.shape == ref.shape == ((2 if mod == 'FSK' else 8), sps)
            assert lut.tobytes() == ref.tobytes(), (mod, sps)


def test_framer_bits_equal_the_reference(gold):
    proto = loadProtocol('CC11xx')(conf=cfg.cc11xx_config())
    enc = proto.getFramer(None)(proto, None)
    for n in (1, 40, 253):
        ref = np.unpackbits(gold[f'frame/{n}/bits'])[:int(gold[f'frame/{n}/nbits'])]
        bits = enc.encodeAndFrame(gold[f'frame/{n}/payload'])
        assert bits.dtype == np.uint8 and np.array_equal(bits, ref), n
    with pytest.raises(DataLengthError):
        enc.encodeAndFrame(np.zeros(254, np.uint8))
    pre, sync = proto.initTxHeader()
    assert len(pre) == 80 and np.array_equal(np.packbits(sync), [0xd6, 0xba, 0xd6, 0xba])
    assert all(len(a) == 0 for a in proto.initTxTail())


def test_protocol_hooks():
    cc = loadProtocol('CC11xx')(conf=cfg.cc11xx_config())
    assert cc.getModulator(None) is modulators.FSKmod
    gm = loadProtocol('bench_GMSK')(conf=cfg.bench_config('bench_GMSK'))
    assert gm.getModulator(None) is modulators.GMSKmod and not hasattr(gm, 'getFramer')


def test_quantisation_corner_values():
    two63 = np.uint64(1) << np.uint64(63)
    for q in (mm.quantise, phase.quantise):
        assert q(0.0) == 0
        assert q(np.pi) == two63                                      # half a turn, exactly
        assert q(-np.pi / 2) == np.uint64(3) << np.uint64(62)         # negative: three quarters of a turn
        assert q(-np.pi) == two63
        assert q(2 * np.pi) == 0
        assert q(-1e-30) == 0                                         # rounds up to a whole turn: the turn 0
        just_under = float(np.nextafter(2 * np.pi, 0))
        assert int(q(just_under)) >= 2 ** 64 - 2 ** 12                # the last or last but one double below a whole turn
        for v in (just_under, 1e6, -1e6, -0.3, 7.0):                  # the rule itself, in Python's exact integers
            t = v / (2 * math.pi)
            frac = t - math.floor(t)
            assert 0 <= frac < 1 and int(q(v)) == int(frac * 2 ** 64), v
        v = np.array([[-0.3, 0.0], [7.0, 1e6]])
        assert q(v).shape == (2, 2) and q(v).dtype == np.uint64
        assert all(q(v)[i, j] == q(v[i, j]) for i in range(2) for j in range(2))


def test_words_by_sample_equal_words_by_symbol_prefix(gold):
    rs = np.random.RandomState(5)
    for mod in ('FSK', 'GMSK'):
        for sps in (2, 5, 16, 128):
            lut = gold[f'lut/{mod}/{sps}']
            for nbits in (2, 3, 65, 300):
                bits = rs.randint(0, 2, nbits)
                for d in (0.0, 0.0123, -2.5):
                    w = mm.words(KIND[mod], lut, bits, d)
                    assert np.array_equal(phase.phase_words(KIND[mod], lut, bits, d), w), (mod, sps, nbits, d)
                    assert np.array_equal(phase.phase_words_by_sample(KIND[mod], lut, bits, d), w)
    assert np.array_equal(phase.phase_words(mm.FSK, gold['lut/FSK/16'], [1]), mm.words(mm.FSK, gold['lut/FSK/16'], [1]))
    with pytest.raises(ValueError):
        phase.phase_words(mm.GMSK3, gold['lut/GMSK/16'], [1])


def test_gmsk_rows_edge_rule():
    assert list(phase.rows_of(phase.GMSK3, [1, 1])) == [3, 6]
    assert list(phase.rows_of(phase.GMSK3, [1, 0, 1, 1])) == [2, 5, 3, 6]
    assert list(phase.rows_of(phase.FSK, [1, 0, 1])) == [1, 0, 1]


def test_host_backend_against_every_golden(gold):
    for mod in ('FSK', 'GMSK'):
        for i in range(int(gold[f'short/{mod}/count'])):
            p = f'short/{mod}/{i}/'
            sps = int(gold[p + 'sps'])
            m = make_modulator(gold, mod, sps, 'host')
            assert m.phaseIncrement() == float(gold[p + 'dphi'])
            m.pad_len = m.min_len = 0
            sig = m.modulate(gold[p + 'bits'])
            assert sig.dtype == np.complex64 and len(sig) == len(gold[p + 'ref'])
            d = comp_dist(sig, gold[p + 'ref'])
            assert d <= mm.BOUND + float(gold[p + 'dist']), (p, d)
        p = f'whole/{mod}/'
        m = make_modulator(gold, mod, 16, 'host')
        sig = m.modulate(gold[p + 'bits'])
        assert sig.dtype == np.complex64 and len(sig) == len(gold[p + 'out'])
        assert comp_dist(sig, gold[p + 'out']) <= mm.BOUND + float(gold[p + 'dist'])
        assert float(gold[f'long/{mod}/dist']) < 1e-5         # recorded, not a waveform: the reference's own float64 drift


def test_pad_layout_is_exact(gold):
    noise = gold['noise']
    for nbits, pre in ((100, 16384 - 8192 - 1600), (512, 0), (511, 16384 - 8192 - 511 * 16), (2000, 0)):
        m = make_modulator(gold, 'FSK', 16, 'host')
        bits = np.arange(nbits) % 3 == 0
        sig = m.modulate(bits)
        L = nbits * 16
        assert mm.layout(L, 4096, 16384) == (pre, pre + L + 8192) == phase.pad_layout(L, 4096, 16384)
        assert len(sig) == pre + L + 8192 and len(sig) >= 16384
        assert sig[:pre].tobytes() == noise[:pre].tobytes()
        assert sig[pre:pre + 4096].tobytes() == noise[:4096].tobytes()
        assert sig[pre + 4096 + L:].tobytes() == noise[:4096].tobytes()
        body = sig[pre + 4096:pre + 4096 + L]
        assert np.abs(np.abs(body) - 1).max() < 1e-6
        w = m.phase_words()[0]
        assert np.array_equal(w, mm.words(mm.FSK, m.modulatorCLS.LUT, bits, m.phaseIncrement()))
        assert body.tobytes() == mm.iq(w).astype(np.complex64).tobytes()
    default = Modulator({}, radio_of(gold, 16), loadProtocol('CC11xx')(conf=cfg.cc11xx_config()), backend='host')
    assert default.noise.dtype == np.complex64 and len(default.noise) == 16384 and 0 < np.abs(default.noise).max() < 1e-6


def test_setters_change_the_increment_as_the_reference_computes_it(gold):
    m = make_modulator(gold, 'FSK', 16, 'host')
    m.set_rangerate(-3210.5)
    m.TxFreqOffset = 1234.5
    m.TxCentreFreqOffset = -77.0
    assert m.get_rangerate() == -3210.5 and m.TxFreqOffset == 1234.5 and m.TxCentreFreqOffset == -77.0
    fc, baud, sps = m.Fc, m.baudRate, 16
    doppler = -3210.5 / 3e8 * fc * 2 * np.pi
    assert m.getDoppler() == doppler
    dopplerCoef = doppler / baud / sps
    offsetCoef = 1234.5 * 2 * np.pi / baud / sps + -77.0 * 2 * np.pi / baud / sps
    assert m.phaseIncrement() == dopplerCoef + offsetCoef
    assert m.phaseIncrement(100.0) == 100.0 / 3e8 * fc * 2 * np.pi / baud / sps + offsetCoef
    assert m.get_samp_rate() == baud * sps and m.TxTotalFreqOffset == 1234.5 - 77.0 + -3210.5 / 3e8 * fc
    assert m.TxFreqOffsetRads == 1234.5 * 2 * np.pi and m.TxCentreFreqOffsetRads == -77.0 * 2 * np.pi
    bits = np.r_[1, 0, 0, 1, 1]
    m.pad_len = m.min_len = 0
    a, b = m.modulate_batch([bits, bits], rangerates=[0.0, 5000.0])
    assert np.array_equal(m.phase_words()[1], mm.words(mm.FSK, m.modulatorCLS.LUT, bits, m.phaseIncrement(5000.0)))
    assert not np.array_equal(a, b)
    frame = m.encodeAndFrame([1, 2, 3])
    assert np.array_equal(m.encodeAndModulate([1, 2, 3]), m.modulate(frame))
    with pytest.raises(RuntimeError):
        m.modulate_device([bits])
    with pytest.raises(ValueError):
        Modulator({}, radio_of(gold, 16), m.protocol, backend='eager')


def test_header_and_binding_surface_match():
    from pycusdr_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'mfbank.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = {n: a for n, a in re.findall(r'\bint\s+(mfb_(?:modulator_[a-z_]+|debug_mod_phase))\s*\(([^)]*)\)', text)}
    expect = {'mfb_modulator_create', 'mfb_modulator_destroy', 'mfb_modulator_set_lut', 'mfb_modulator_set_pad', 'mfb_modulator_begin',
              'mfb_modulator_end', 'mfb_modulator_device_output', 'mfb_modulator_host_buffer', 'mfb_debug_mod_phase'}
    assert set(declared) == expect
    for name, args in declared.items():
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is _lib._i and len(argtypes) == len(args.split(',')), name
    assert re.search(r'#define\s+MFB_MOD_FSK\s+0', text) and re.search(r'#define\s+MFB_MOD_GMSK3\s+1', text)
    assert (phase.FSK, phase.GMSK3) == (0, 1)
    pkg = os.path.join(ROOT, 'pycusdr_amd', 'modulator')
    for f in os.listdir(pkg):
        if f.endswith('.py'):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r'^\s*(from|import)\s+(oracle|tests|modulator_model)\b', src, flags=re.M), f
