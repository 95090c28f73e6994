"""Modulator -> wideband channel -> rational plan on the raster -> receive loop, all on the device: two downlinks on raster slots of
one capture whose rate is 25/16 of the bank's, each received by its own ``DemodulatorRunner.run_device_stream`` from its own
``ChannelizerSource`` on one ``UniformChannelizer(interp=16)``.  The geometry of test_gpu_channelizer_rational_loopback.py on the
raster of test_gpu_channelizer_uniform_loopback.py."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.channel import Channel
from pycusdr_amd.channelizer import ChannelizerSource, ChannelWide, UniformChannelizer, design_taps, uniform_rate
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu


def test_two_raster_slots_at_25_16_of_the_bank_rate_each_reach_their_own_receiver():
    """CC11xx, 2^17 x 64 bins, 128 samples per symbol at the bank, 4 blocks per window, 3 windows.  The frames are modulated at 200
    samples per symbol, the capture rate is baud * 200; (U, D) = (16, 25) with design_taps(25, interp=16) (401 taps) brings every
    bin of an 8-bin raster to the bank's rate.  The frames sit at different times on the bin centres +fs/8 and -3fs/8, 15 dB
    there: bins 1 and 5, the only two selected, half the capture rate apart because these taps pass 0.256 fs to either side of a
    centre.  Each runner returns exactly its own frame's packet, CRC good, the payload sent."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps, wsps, B, nwin, M = 17, 128, 200, 4, 3, 8
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
    U, D = uniform_rate(fs, baud * sps, M)
    assert (U, D) == (16, 25)
    tx = Modulator(wconf, wradio, wp, backend='hip')
    tx.set_rangerate(0.0)
    payloads = [np.arange(1, 41, dtype=np.uint8), np.arange(200, 160, -1).astype(np.uint8)]
    batch = tx.modulate_device([tx.encodeAndFrame(pl) for pl in payloads])
    length = batch.frame_len(0)
    assert length == batch.frame_len(1) >= (10 + 4 + 1 + 40 + 2) * 8 * wsps

    taps = design_taps(D, interp=U)
    assert len(taps) == 401
    carriers = (fs / 8, -3 * fs / 8)
    packets = []
    runs = [DemodulatorRunner(conf, p, 'UHF-H') for _ in range(2)]
    ov = runs[0].overlap
    step = N - ov
    count = B * step + ov
    max_in = -(-count * D // U) + 64
    chan = Channel(fs, seed=77, backend='hip', max_samples=max_in, max_source=batch.total)
    chan.set_source(batch)
    # at the wide rate: the first frame inside window 0, the second across the boundary of windows 1 and 2
    starts = ((ov + 60000) * D // U, (2 * B * step - 20000) * D // U)
    assert starts[0] + length < starts[1] and starts[1] < 2 * B * step * D // U < starts[1] + length
    assert starts[0] + length < B * step * D // U
    frames = [chan.frame(starts[f], int(batch.sample_off[f]), length, 1.0, carriers[f], 0.0, 0.3 * f) for f in range(2)]
    wide = ChannelWide(chan, frames, sigma=chan.sigma_for(15.0, power=1.0))
    cz = UniformChannelizer(fs, M, D, taps, bins=[1, 5], max_in=max_in, max_out=count, interp=U)
    assert np.array_equal(cz.freqs_hz, carriers) and cz.K == 2 and cz.rational
    for k in range(2):
        src = ChannelizerSource(cz, k, wide, N, ov, B, nwin)
        res, pk = runs[k].run_device_stream(src, decoder=Decoder({}, p))
        runs[k].close()
        assert len(res) == B * nwin and [d['count'] for d in res] == list(range(B * nwin))
        packets.append(pk)
    cz.close()
    chan.close()
    tx.close()
    for k in range(2):
        assert len(packets[k]) == 1, (k, len(packets[k]))       # its own frame, nothing of the other channel's
        data, crc_err, _ = packets[k][0].getBinaryData()
        assert packets[k][0].packetLen == 42 and not crc_err and np.array_equal(data[:-2], payloads[k]), k
