"""``Modulator``: framing (the protocol's framer) and LUT modulation (the protocol's modulator) with the Doppler and
frequency offsets of an uplink pre-compensated, as the reference's class of that name (modulator/modulator.py:34-212).

Two back ends compute the same uint64 phase words (phase.py): ``'hip'`` runs csrc/mod_kernels.hpp through the
mfb_modulator_* handle, whole batches of frames per device call; ``'host'`` is numpy.  There is no fall-back from one to
the other: ``'hip'`` without the library or a GPU raises.

Where the reference adds Doppler and offsets to every entry of the table in float64 and sums the result, the table is
quantised here once and the frame's increment -- dopplerCoef + offsetCoef, one double -- separately; the two differ by
less than 2**-63 turns per sample.  Not built: the ZeroMQ transport around the reference's class
(modulator_process.py).
"""
import numpy as np

from . import phase
from .device import MAX_BITS, MAX_SAMPLES, DeviceModulator

SIG_MIN_LENGTH = 16384      # shorter signals are pre-padded to this (modulator.py:27, 121-123)
NOISE_LEN = 4096            # samples of tiny noise in front of and behind every frame (modulator.py:29, 117-118)
NOISE_VAR = 0.00000001


def _pow2ceil(n):
    p = 1
    while p < n:
        p <<= 1
    return p


class Modulator:
    def __init__(self, conf, confRadio, protocol, backend='hip', noise=None, device=0):
        if backend not in ('hip', 'host'):
            raise ValueError(f'unknown backend {backend!r}')
        self.conf, self.confRadio, self.protocol, self.backend, self.device = conf, confRadio, protocol, backend, device
        framer = protocol.getFramer(confRadio) if hasattr(protocol, 'getFramer') else None
        self.encoder = framer(protocol, confRadio) if framer else None
        self.modulatorCLS = protocol.getModulator(confRadio)(protocol, confRadio)
        self._spSym = confRadio['samplesPerSym']
        self.Fc = confRadio['frequency_Hz']
        self._TxFreqOffset = confRadio['frequencyOffset_Hz']
        self._TxCentreFreqOffset = confRadio.get('centreFrequencyOffset', 0.)
        self.baudRate = confRadio['baud']
        if noise is None:      # made once per Modulator, as the reference does (modulator.py:77)
            noise = NOISE_VAR * (np.random.randn(SIG_MIN_LENGTH) + 1j * np.random.randn(SIG_MIN_LENGTH))
        self.noise = np.asarray(noise).astype(np.complex64)
        self.pad_len, self.min_len = NOISE_LEN, SIG_MIN_LENGTH
        if len(self.noise) < max(self.pad_len, self.min_len):
            raise ValueError('the noise array is shorter than the pads it fills')
        self._rangerate = 0
        self._dev = None
        self._last = None      # ('host', [words per frame]) of the last batch, for phase_words()

    # ---- framing -----------------------------------------------------------------------------------------------------------
    def encodeAndFrame(self, byteMessage):
        if self.encoder is None:
            raise NotImplementedError(f'{self.protocol.name} has no framer')
        return self.encoder.encodeAndFrame(byteMessage)

    def encodeAndModulate(self, byteMessage):
        return self.modulate(self.encodeAndFrame(byteMessage))

    # ---- modulation --------------------------------------------------------------------------------------------------------
    def phaseIncrement(self, rangerate=None):
        """dopplerCoef + offsetCoef of modulator.py:103-108, rad per sample, for ``rangerate`` (default: the current one)."""
        rr = self._rangerate if rangerate is None else rangerate
        dopplerCoef = rr / 3e8 * self.Fc * 2 * np.pi / self.baudRate / self.spSym
        freqOffset = self.TxFreqOffsetRads / self.baudRate / self.spSym
        centreFreqOffset = self.TxCentreFreqOffsetRads / self.baudRate / self.spSym
        return dopplerCoef + (freqOffset + centreFreqOffset)

    def modulate(self, bitData):
        return self.modulate_batch([bitData])[0]

    def modulate_batch(self, frames, rangerates=None):
        """Every frame of the list modulated in one device call, frame f with the Doppler of ``rangerates[f]`` (default: the
        current range rate for all).  Returns the list of complex64 arrays, pads included."""
        frames, dphi = self._prepare(frames, rangerates)
        if self.backend == 'host':
            words = [phase.phase_words(self.modulatorCLS.kind, self.modulatorCLS.LUT, b, d) for b, d in zip(frames, dphi)]
            self._last = words
            return [phase.assemble(phase.words_to_iq(w).astype(np.complex64), self.noise, self.pad_len, self.min_len) for w in words]
        dev = self._device_for(frames)
        dev.begin(frames, dphi)
        sig, off = dev.end(copy=True)
        return [sig[off[f]:off[f + 1]] for f in range(len(frames))]

    def modulate_device(self, frames, rangerates=None):
        """As modulate_batch, but the batch stays on the device: a DeviceBatch whose ``frame_ptr(f)`` is what
        ``mfb_upload_device`` / ``MFBank.upload_device`` takes.  Valid until this modulator's next call."""
        if self.backend != 'hip':
            raise RuntimeError("modulate_device needs backend='hip'")
        frames, dphi = self._prepare(frames, rangerates)
        dev = self._device_for(frames)
        dev.begin(frames, dphi)
        return dev.end(copy=False)

    def phase_words(self):
        """The uint64 phase words of the last batch, per frame, without the pads (on 'hip' through mfb_debug_mod_phase)."""
        if self.backend == 'host':
            return self._last
        words = self._dev.phase_words()
        out, pos = [], 0
        for n in self._last:
            pre, total = phase.pad_layout(n, self.pad_len, self.min_len)
            out.append(words[pos + pre + self.pad_len:pos + pre + self.pad_len + n])
            pos += total
        return out

    def _prepare(self, frames, rangerates):
        frames = [np.asarray(f).reshape(-1) for f in frames]
        if not frames:
            raise ValueError('no frames')
        for f in frames:
            if len(f) < self.modulatorCLS.min_bits:
                raise ValueError(f'{self.modulatorCLS.name} needs at least {self.modulatorCLS.min_bits} bits per frame')
        if rangerates is None:
            rangerates = [self._rangerate] * len(frames)
        if len(rangerates) != len(frames):
            raise ValueError('one range rate per frame')
        return frames, np.array([self.phaseIncrement(rr) for rr in rangerates], dtype=np.float64)

    def _device_for(self, frames):
        nbits = sum(len(f) for f in frames)
        nsamp = sum(phase.pad_layout(len(f) * self.spSym, self.pad_len, self.min_len)[1] for f in frames)
        self._last = [len(f) * self.spSym for f in frames]
        if self._dev is None or nbits > self._dev.max_bits or nsamp > self._dev.max_samples:
            if self._dev is not None:
                self._dev.close()
            self._dev = DeviceModulator(min(max(_pow2ceil(nbits), 1 << 12), max(MAX_BITS, nbits)),
                                        min(max(_pow2ceil(nsamp), 1 << 16), max(MAX_SAMPLES, nsamp)), self.device)
            self._dev.set_lut(self.modulatorCLS.kind, self.modulatorCLS.LUT)
            self._dev.set_pad(self.noise, self.pad_len, self.min_len)
        return self._dev

    def close(self):
        if self._dev is not None:
            self._dev.close()
            self._dev = None

    # ---- setters and getters (modulator.py:141-212) -------------------------------------------------------------------------
    def get_rangerate(self):
        return self._rangerate

    def set_rangerate(self, rangerate):
        self._rangerate = rangerate

    def getDoppler(self):
        """rad per second"""
        return self._rangerate / 3e8 * self.Fc * 2 * np.pi

    def get_samp_rate(self):
        return self.baudRate * self._spSym

    def get_Tx_Fc(self):
        return self.Fc

    def set_Tx_Fc(self, Fc):
        self.Fc = Fc

    @property
    def spSym(self):
        return self._spSym

    @property
    def TxTotalFreqOffset(self):
        return self._TxFreqOffset + self._TxCentreFreqOffset + self._rangerate / 3e8 * self.Fc

    @property
    def TxFreqOffset(self):
        return self._TxFreqOffset

    @TxFreqOffset.setter
    def TxFreqOffset(self, fo):
        self._TxFreqOffset = fo

    @property
    def TxFreqOffsetRads(self):
        return self._TxFreqOffset * 2 * np.pi

    @property
    def TxCentreFreqOffset(self):
        return self._TxCentreFreqOffset

    @TxCentreFreqOffset.setter
    def TxCentreFreqOffset(self, offset):
        self._TxCentreFreqOffset = offset

    @property
    def TxCentreFreqOffsetRads(self):
        return self._TxCentreFreqOffset * 2 * np.pi
