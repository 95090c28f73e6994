"""Modulator -> synthesiser -> wideband channel -> uniform polyphase channeliser -> receive loop, all on the device and each at its
own rate: two downlinks modulated at the narrow rate, put on raster slots of one wideband stream by ``UniformSynthesizer``, each
received by its own ``DemodulatorRunner.run_device_stream`` from its own ``ChannelizerSource`` on a ``UniformChannelizer``.  The
geometry of test_gpu_channelizer_uniform_loopback.py, without modulating at the wide rate."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.channel import Channel
from pycusdr_amd.channelizer import ChannelizerSource, UniformChannelizer, design_taps
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol
from pycusdr_amd.synthesizer import SynthesizerWide, UniformSynthesizer

pytestmark = pytest.mark.gpu


def test_two_narrow_frames_on_raster_slots_each_reach_their_own_receiver():
    """CC11xx, 2^17 x 64 bins, 128 samples per symbol, 4 blocks per window, 3 windows.  The frames are modulated at 128 samples per
    symbol and placed at different times on bins 2 and 6 of an 8-bin raster (+fs/4 and -fs/4) with I = 4 and 4 design_taps(4); the
    wide stream passes a Channel at 15 dB; D = 4 with design_taps(4) takes the two bins out again.  Each runner returns exactly
    its own frame's packet."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps, B, nwin, D = 17, 128, 4, 3, 4
    N = 1 << bs
    conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps)
    p = loadProtocol('CC11xx')(conf=conf)
    p.CRC_CHECK = 'framer'
    radio = conf['Radios']['Rx']['UHF-H']
    fs = float(radio['baud'] * sps * D)
    tx = Modulator(conf, radio, p, backend='hip')
    tx.set_rangerate(0.0)
    payloads = [np.arange(1, 41, dtype=np.uint8), np.arange(200, 160, -1).astype(np.uint8)]
    batch = tx.modulate_device([tx.encodeAndFrame(pl) for pl in payloads])
    length = batch.frame_len(0)
    assert length == batch.frame_len(1) == (10 + 4 + 1 + 40 + 2) * 8 * sps + 8192 == 66560

    taps = design_taps(D)
    assert len(taps) == 65
    packets = []
    runs = [DemodulatorRunner(conf, p, 'UHF-H') for _ in range(2)]
    ov = runs[0].overlap
    step = N - ov
    count = B * step + ov
    max_in = count * D + 64
    syn = UniformSynthesizer(fs, 8, D, (D * taps.astype(np.float64)).astype(np.float32), max_out=max_in, max_source=batch.total)
    syn.set_source(batch)
    # at the narrow rate: the first frame inside window 0, the second across the boundary of windows 1 and 2
    starts = (ov + 60000, 2 * B * step - 20000)
    assert starts[0] + length < starts[1] and starts[1] < 2 * B * step < starts[1] + length
    placements = [syn.placement(b, starts[f], int(batch.sample_off[f]), length) for f, b in enumerate((2, -2))]
    assert [q.bin for q in placements] == [2, 6]
    chan = Channel(fs, seed=77, backend='hip', max_samples=max_in)
    wide = SynthesizerWide(syn, placements, channel=chan, sigma=chan.sigma_for(15.0, power=1.0))
    cz = UniformChannelizer(fs, 8, D, taps, bins=[2, 6], max_in=max_in, max_out=count)
    assert np.array_equal(cz.freqs_hz, (fs / 4, -fs / 4)) and np.array_equal(syn.freqs_hz[[2, 6]], cz.freqs_hz)
    for k in range(2):
        src = ChannelizerSource(cz, k, wide, N, ov, B, nwin)
        res, pk = runs[k].run_device_stream(src, decoder=Decoder({}, p))
        runs[k].close()
        assert len(res) == B * nwin and [d['count'] for d in res] == list(range(B * nwin))
        packets.append(pk)
    cz.close()
    chan.close()
    syn.close()
    tx.close()
    for k in range(2):
        assert len(packets[k]) == 1, (k, len(packets[k]))       # its own frame, nothing of the other channel's
        data, crc_err, _ = packets[k][0].getBinaryData()
        assert packets[k][0].packetLen == 42 and not crc_err and np.array_equal(data[:-2], payloads[k]), k
