#!/usr/bin/env python3
"""Generate ``ref_goldens_modulator.npz`` from the reference's transmit side (pyCuSDR/modulator/, found where make_golden.py
finds the reference).

Test infrastructure, like make_golden.py, whose import shims it reuses: it runs only where the reference exists; its
output is data (inputs and recorded results) and is what tests/test_modulator_host.py and tests/test_gpu_modulator.py read.

  lut/<GMSK|FSK>/<spSym>       the reference's GMSKmod.LUT / FSKmod.LUT, float64, spSym 2, 5, 16, 128
  frame/<n>/payload, bits      the reference's CC11xx encodeAndFrame for payloads of 1, 40 and 253 bytes
  short/<mod>/<i>/...          modulatorCLS.modulate(bits, LUT + dopplerCoef + offsetCoef) of short frames with a non-zero
                               range rate and offset: bits, spSym, the increment dphi = dopplerCoef + offsetCoef, the output
                               (float64 for GMSK; FSKmod casts to complex64 itself) and dist, the largest per-component
                               distance of the integer model (tests/modulator_model.py) from it
  whole/<mod>/...              one whole Modulator.modulate, pads included, with the numbers of its radio and the noise
  noise                        the 16384 noise samples both used
  long/<mod>/dist              10 000 bits x 16 samples per symbol: only the model's distance from the reference

The file is refused if any short or whole case's distance exceeds 1e-6 or if a table rebuilt by
pycusdr_amd/modulator/modulators.py differs from the reference's in any bit.

Usage:  python tests/golden/make_golden_modulator.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from make_golden import _install_shims  # noqa: E402

SPS = (2, 5, 16, 128)
SHORT = {'GMSK': [(2, 2), (3, 5), (65, 16), (257, 5), (8, 128)], 'FSK': [(1, 16), (2, 2), (3, 5), (65, 16), (257, 5), (8, 128)]}
RADIO = {'frequency_Hz': 401.538e6, 'frequencyOffset_Hz': 148320, 'baud': 7416, 'centreFrequencyOffset': -312.5}
RANGERATE = 6100.0
LIMIT = 1e-6


def dist(a, b):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return float(max(np.abs(a.real - b.real).max(), np.abs(a.imag - b.imag).max()))


def main():
    _install_shims()
    import modulator as refmod
    from modulator.modulators import FSKmod, GMSKmod
    from protocol.CC11xx import CC11xx as RefCC11xx
    import modulator_model as mm
    from pycusdr_amd import config as cfg
    from pycusdr_amd.modulator import modulators as ours

    out = {}
    rs = np.random.RandomState(2027)
    classes = {'GMSK': (GMSKmod, ours.GMSKmod, mm.GMSK3), 'FSK': (FSKmod, ours.FSKmod, mm.FSK)}

    def radio(sps):
        return dict(RADIO, samplesPerSym=sps)

    def ref_modulator(mod, sps):
        """The reference's Modulator around one of its LUT classes, without the framer its constructor insists on."""
        m = object.__new__(refmod.Modulator)
        m.modulatorCLS = classes[mod][0](None, radio(sps))
        m._spSym, m.Fc, m.baudRate = sps, RADIO['frequency_Hz'], RADIO['baud']
        m._TxFreqOffset, m._TxCentreFreqOffset = RADIO['frequencyOffset_Hz'], RADIO['centreFrequencyOffset']
        m._rangerate = RANGERATE
        return m

    def increments(m):
        """dopplerCoef, offsetCoef as modulator.py:103-108 computes them"""
        dopplerCoef = m.getDoppler() / m.baudRate / m.spSym
        offsetCoef = m.TxFreqOffsetRads / m.baudRate / m.spSym + m.TxCentreFreqOffsetRads / m.baudRate / m.spSym
        return dopplerCoef, offsetCoef

    for mod, (ref_cls, our_cls, kind) in classes.items():
        for sps in SPS:
            lut = ref_cls(None, radio(sps)).LUT
            assert lut.dtype == np.float64
            mine = our_cls(None, radio(sps)).LUT
            assert mine.shape == lut.shape and mine.tobytes() == lut.tobytes(), f'{mod} LUT at spSym {sps} differs from the reference'
            out[f'lut/{mod}/{sps}'] = lut

    conf = cfg.cc11xx_config()
    proto = RefCC11xx(conf=conf)
    enc = proto.getFramer(None)(proto, None)
    for n in (1, 40, 253):
        payload = rs.randint(0, 256, n).astype(np.uint8)
        bits = np.asarray(enc.encodeAndFrame(payload.copy()))
        assert set(np.unique(bits)) <= {0, 1}
        out[f'frame/{n}/payload'] = payload
        out[f'frame/{n}/bits'] = np.packbits(bits.astype(np.uint8))
        out[f'frame/{n}/nbits'] = np.int64(len(bits))

    for mod, (ref_cls, our_cls, kind) in classes.items():
        for i, (nbits, sps) in enumerate(SHORT[mod]):
            m = ref_modulator(mod, sps)
            dc, oc = increments(m)
            bits = rs.randint(0, 2, nbits).astype(np.int64)
            sig = m.modulatorCLS.modulate(bits, m.modulatorCLS.LUT + dc + oc)
            model = mm.iq(mm.words(kind, m.modulatorCLS.LUT, bits, dc + oc))
            d = dist(model, sig)
            print(f'short {mod} {nbits} bits x {sps}: dist {d:.3e} ({sig.dtype})')
            assert d <= LIMIT, (mod, nbits, sps, d)
            p = f'short/{mod}/{i}/'
            out[p + 'bits'] = bits.astype(np.uint8)
            out[p + 'sps'] = np.int64(sps)
            out[p + 'dphi'] = np.float64(dc + oc)
            out[p + 'ref'] = sig
            out[p + 'dist'] = np.float64(d)
        out[f'short/{mod}/count'] = np.int64(len(SHORT[mod]))

    noise = (1e-8 * (rs.randn(16384) + 1j * rs.randn(16384))).astype(np.complex64)
    out['noise'] = noise
    out['radio'] = np.array([RADIO['frequency_Hz'], RADIO['frequencyOffset_Hz'], RADIO['baud'], RADIO['centreFrequencyOffset'], RANGERATE])
    frame40 = np.unpackbits(out['frame/40/bits'])[:int(out['frame/40/nbits'])]
    for mod, bits in (('FSK', frame40.astype(np.int64)), ('GMSK', rs.randint(0, 2, 600).astype(np.int64))):
        m = ref_modulator(mod, 16)
        m.noise = noise
        sig = m.modulate(bits)
        assert sig.dtype == np.complex64
        dc, oc = increments(m)
        kind = classes[mod][2]
        model = mm.frame(mm.iq(mm.words(kind, m.modulatorCLS.LUT, bits, dc + oc)), noise, 4096, 16384)
        assert len(model) == len(sig), (len(model), len(sig))
        d = dist(model, sig)
        print(f'whole {mod} {len(bits)} bits x 16 -> {len(sig)} samples: dist {d:.3e}')
        assert d <= LIMIT
        p = f'whole/{mod}/'
        out[p + 'bits'] = bits.astype(np.uint8)
        out[p + 'sps'] = np.int64(16)
        out[p + 'dphi'] = np.float64(dc + oc)
        out[p + 'out'] = sig
        out[p + 'dist'] = np.float64(d)

    for mod, (ref_cls, our_cls, kind) in classes.items():
        m = ref_modulator(mod, 16)
        dc, oc = increments(m)
        bits = rs.randint(0, 2, 10000).astype(np.int64)
        sig = m.modulatorCLS.modulate(bits, m.modulatorCLS.LUT + dc + oc)
        d = dist(mm.iq(mm.words(kind, m.modulatorCLS.LUT, bits, dc + oc)), sig)
        print(f'long {mod}: dist {d:.3e}')
        out[f'long/{mod}/dist'] = np.float64(d)

    path = os.path.join(HERE, 'ref_goldens_modulator.npz')
    np.savez_compressed(path, **{k.replace('/', '__'): v for k, v in out.items()})
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 768 << 10


if __name__ == '__main__':
    main()
