"""Framers of the transmit side: payload bytes -> the bits to modulate.

``CC11xx`` builds the frame of the reference's encoder of that name (modulator/encoders/CC11xx.py:31-134): length byte
(payload + 2, it counts the CRC), CRC-16 low byte first, PN9 whitening of all of that, then preamble and sync from the
protocol (initTxHeader).  The bench protocols have no framer: the reference's ``bench_base.getFramer`` names an
encoder class that is not in its tree.
"""
import numpy as np

from ..protocol.CC11xx import crc16_cc11xx, pn9_bytes

MAX_TX_DATA_LEN = 255      # the length byte; the reference tests against 256 and would then write a length of 0


class DataLengthError(ValueError):
    """The payload does not fit the frame's length field."""


class Encoder:
    name = 'base'

    def __init__(self, protocol, confRadio):
        self.protocol = protocol

    def encodeAndFrame(self, data):
        return data


class CC11xx(Encoder):
    name = 'CC11xx'

    def __init__(self, protocol, confRadio):
        super().__init__(protocol, confRadio)
        self.whiten = protocol.whiten
        self.Flags, self.Header = protocol.initTxHeader()
        self.TailFlags, self.Tail = protocol.initTxTail()

    def encodeAndFrame(self, data):
        data = np.asarray(data).astype(np.uint8).reshape(-1)
        dataLen = len(data) + 2
        if dataLen > MAX_TX_DATA_LEN:
            raise DataLengthError(f'TX maximum allowed data length {MAX_TX_DATA_LEN} bytes. Got {dataLen} bytes')
        body = np.r_[np.uint8(dataLen), data]
        crc = crc16_cc11xx(body)
        body = np.r_[body, np.uint8(crc & 0xFF), np.uint8(crc >> 8)]
        if self.whiten:
            body = np.bitwise_xor(body, pn9_bytes(len(body)).astype(np.uint8))
        return np.r_[self.Flags, self.Header, np.unpackbits(body)].astype(np.uint8)
