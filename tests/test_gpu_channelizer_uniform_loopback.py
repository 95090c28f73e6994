"""Modulator -> wideband channel -> uniform polyphase channeliser -> receive loop, all on the device: two downlinks on raster slots
of one wideband capture, each received by its own ``DemodulatorRunner.run_device_stream`` from its own ``ChannelizerSource`` on a
``UniformChannelizer``.  The geometry of test_gpu_channelizer_loopback.py."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.channel import Channel
from pycusdr_amd.channelizer import ChannelizerSource, ChannelWide, UniformChannelizer, design_taps
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu


def test_two_raster_slots_of_one_capture_each_reach_their_own_receiver():
    """CC11xx, 2^17 x 64 bins, 128 samples per symbol at the narrow rate, 4 blocks per window, 3 windows; D = 4 with
    design_taps(4) (65 taps).  The frames are modulated at 512 samples per symbol (same baud) and placed at different times on
    the carriers +fs/4 and -fs/4 of the capture, 15 dB there: bins 2 and 6 of an 8-bin raster, the only two selected.  Each runner
    returns exactly its own frame's packet."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps, B, nwin, D = 17, 128, 4, 3, 4
    N = 1 << bs
    conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps)
    p = loadProtocol('CC11xx')(conf=conf)
    p.CRC_CHECK = 'framer'
    wconf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps * D)
    wp = loadProtocol('CC11xx')(conf=wconf)
    wradio = wconf['Radios']['Rx']['UHF-H']
    fs = float(wradio['baud'] * sps * D)
    assert wradio['baud'] == conf['Radios']['Rx']['UHF-H']['baud']
    tx = Modulator(wconf, wradio, wp, backend='hip')
    tx.set_rangerate(0.0)
    payloads = [np.arange(1, 41, dtype=np.uint8), np.arange(200, 160, -1).astype(np.uint8)]
    batch = tx.modulate_device([tx.encodeAndFrame(pl) for pl in payloads])
    length = batch.frame_len(0)
    assert length == batch.frame_len(1) == (10 + 4 + 1 + 40 + 2) * 8 * sps * D + 8192 == 241664

    taps = design_taps(D)
    assert len(taps) == 65
    carriers = (fs / 4, -fs / 4)
    packets = []
    runs = [DemodulatorRunner(conf, p, 'UHF-H') for _ in range(2)]
    ov = runs[0].overlap
    step = N - ov
    count = B * step + ov
    max_in = count * D + 64
    chan = Channel(fs, seed=77, backend='hip', max_samples=max_in, max_source=batch.total)
    chan.set_source(batch)
    # at the wide rate: the first frame inside window 0, the second across the boundary of windows 1 and 2
    starts = (D * (ov + 60000), D * (2 * B * step - 20000))
    assert starts[0] + length < starts[1] and starts[1] < D * 2 * B * step < starts[1] + length
    frames = [chan.frame(starts[f], int(batch.sample_off[f]), length, 1.0, carriers[f], 0.0, 0.3 * f) for f in range(2)]
    wide = ChannelWide(chan, frames, sigma=chan.sigma_for(15.0, power=1.0))
    cz = UniformChannelizer(fs, 8, D, taps, bins=[2, 6], max_in=max_in, max_out=count)
    assert np.array_equal(cz.freqs_hz, carriers) and cz.K == 2
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
