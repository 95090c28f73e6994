"""Modulator -> wideband channel -> rational channeliser -> receive loop, all on the device: one downlink on a carrier of a capture
whose rate is 25/16 of the bank's, received by ``DemodulatorRunner.run_device_stream`` from a ``ChannelizerSource`` over a plan
with ``interp = 16``.  The geometry of test_gpu_channelizer_loopback.py."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.channel import Channel
from pycusdr_amd.channelizer import Channelizer, ChannelizerSource, ChannelWide, design_taps, factor_rate
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu


def test_a_downlink_at_25_16_of_the_bank_rate_reaches_the_receiver():
    """CC11xx, 2^17 x 64 bins, 128 samples per symbol at the bank, 4 blocks per window, 3 windows.  The frame is modulated at 200
    samples per symbol, the capture rate is baud * 200, the frame sits on the carrier +fs/5 at 15 dB; (U, D) = (16, 25) with
    design_taps(25, interp=16) (401 taps) brings it to the bank's rate.  Exactly one packet, CRC good, the payload sent."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps, wsps, B, nwin = 17, 128, 200, 4, 3
    N = 1 << bs
    conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps)
    p = loadProtocol('CC11xx')(conf=conf)
    p.CRC_CHECK = 'framer'
    wconf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=wsps)
    wp = loadProtocol('CC11xx')(conf=wconf)
    wradio = wconf['Radios']['Rx']['UHF-H']
    baud = wradio['baud']
    assert baud == conf['Radios']['Rx']['UHF-H']['baud']
    fs = float(baud * wsps)
    (U, D), = factor_rate(fs, baud * sps)
    assert (U, D) == (16, 25)
    tx = Modulator(wconf, wradio, wp, backend='hip')
    tx.set_rangerate(0.0)
    payload = np.arange(1, 41, dtype=np.uint8)
    batch = tx.modulate_device([tx.encodeAndFrame(payload)])
    length = batch.frame_len(0)
    assert length >= (10 + 4 + 1 + 40 + 2) * 8 * wsps

    taps = design_taps(D, interp=U)
    assert len(taps) == 401
    carrier = fs / 5
    run = DemodulatorRunner(conf, p, 'UHF-H')
    ov = run.overlap
    step = N - ov
    count = B * step + ov
    max_in = -(-count * D // U) + 64
    chan = Channel(fs, seed=77, backend='hip', max_samples=max_in, max_source=batch.total)
    chan.set_source(batch)
    # at the wide rate: the frame across the boundary of windows 0 and 1
    start = (B * step - 20000) * D // U
    assert start < B * step * D // U < start + length
    frames = [chan.frame(start, int(batch.sample_off[0]), length, 1.0, carrier, 0.0, 0.3)]
    wide = ChannelWide(chan, frames, sigma=chan.sigma_for(15.0, power=1.0))
    cz = Channelizer(fs, D, taps, [carrier], max_in=max_in, max_out=count, interp=U)
    src = ChannelizerSource(cz, 0, wide, N, ov, B, nwin)
    res, packets = run.run_device_stream(src, decoder=Decoder({}, p))
    run.close()
    cz.close()
    chan.close()
    tx.close()
    assert len(res) == B * nwin and [d['count'] for d in res] == list(range(B * nwin))
    assert len(packets) == 1, len(packets)
    data, crc_err, _ = packets[0].getBinaryData()
    assert packets[0].packetLen == 42 and not crc_err and np.array_equal(data[:-2], payload)
