"""The LUT modulators: tables of phase increments (rad per sample) per symbol neighbourhood.

``FSKmod`` and ``GMSKmod`` build the same float64 tables as the reference's classes of those names
(modulator/modulators/FSK_LUT.py:9-21, GMSK_LUT.py:10-47; pinned bit for bit by tests/test_modulator_host.py) and
modulate through the integer phase of ``phase.py``.  The reference's third class, ``GFSK2mod``, cannot be constructed
there (its module never imports the Gaussian filter it calls) and is not built here.
"""
import numpy as np

from ..lib.filters import gaussianFilter
from . import phase


class BaseLUT:
    """A modulation is its table ``LUT`` float64 [rows][spSym] and the rule ``kind`` that picks a row per symbol."""
    name = 'base'
    kind = None
    min_bits = 1

    def getLUT(self):
        return self.LUT

    def modulate(self, bitData, symTransLUTDopp):
        """Signature of the reference (the table already carries Doppler and offsets): complex128, float64 evaluation of
        the integer phase."""
        return phase.words_to_iq(phase.phase_words(self.kind, symTransLUTDopp, bitData))


class FSKmod(BaseLUT):
    """2-FSK, tone spacing baud / 2: -pi / spSym per sample for a 0, +pi / spSym for a 1."""
    name = 'FSK'
    kind = phase.FSK

    def __init__(self, protocol, confRadio):
        self.spSym = spSym = confRadio['samplesPerSym']
        wavePhase = np.ones(spSym) / spSym * 2 * np.pi * 0.5
        self.LUT = np.array([-wavePhase, wavePhase])


class GMSKmod(BaseLUT):
    """GMSK, BT 0.5: one pulse per 3-bit neighbourhood -- the middle symbol of the NRZ triple through a Gaussian filter
    convolved with a one-symbol square, scaled so that an isolated run advances pi / 2 per symbol."""
    name = 'GMSK'
    kind = phase.GMSK3
    min_bits = 2

    def __init__(self, protocol, confRadio):
        self.spSym = spSym = confRadio['samplesPerSym']
        filt = np.convolve(gaussianFilter(1, 0.5, spSym, 4 * spSym), np.ones(spSym))
        grpT = int(len(filt) / 2)
        first = np.r_[1, np.zeros(spSym - 1)]
        lut = np.zeros((8, spSym))
        for r in range(8):
            nrz = np.array([(r >> 2) & 1, (r >> 1) & 1, r & 1]) * 2 - 1
            shaped = np.convolve(filt, np.kron(nrz, first))
            lut[r] = shaped[grpT + int(spSym / 2):grpT + int(1.5 * spSym)] * np.pi / 2 / spSym
        self.LUT = lut
