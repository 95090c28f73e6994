"""Modulator -> channel -> receive loop without a trip through host memory (``DemodulatorRunner.run_device_stream`` on the windows
of ``channel.LoopbackSource``), and the same windows fed through the host loop."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.channel import Channel, LoopbackSource
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu


def test_loopback_cc11xx_two_frames_with_sweeps_device_equals_host_fed():
    """The geometry of test_loopback_cc11xx_with_doppler_and_offset: 2^17 x 64 bins, 128 samples per symbol; 4 blocks per window,
    3 windows.  Two frames from modulate_device, the first across the boundary of windows 0 and 1, each on its own Doppler with a
    sweep that stays under one bin spacing over the frame, 15 dB."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps, B, nwin = 17, 128, 4, 3
    N = 1 << bs
    conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps)
    p = loadProtocol('CC11xx')(conf=conf)
    p.CRC_CHECK = 'framer'
    radio = conf['Radios']['Rx']['UHF-H']
    fs = float(radio['baud'] * sps)
    tx = Modulator(conf, radio, p, backend='hip')
    tx.set_rangerate(0.0)
    payloads = [np.arange(1, 41, dtype=np.uint8), np.arange(200, 160, -1).astype(np.uint8)]
    batch = tx.modulate_device([tx.encodeAndFrame(pl) for pl in payloads])
    length = batch.frame_len(0)
    assert length == batch.frame_len(1) == (10 + 4 + 1 + 40 + 2) * 8 * sps + 8192

    run = DemodulatorRunner(conf, p, 'UHF-H')
    ov = run.overlap
    step = N - ov
    spacing = float(np.abs(np.diff(run.demod.doppHzLUT)).max())
    dur = length / fs
    doppler = (2000.0, -3500.0)
    rate = (0.6 * spacing / dur, -0.8 * spacing / dur)
    starts = (B * step - 30000, 2 * B * step + 20000)
    assert starts[0] < B * step < starts[0] + length              # across the boundary of windows 0 and 1
    chan = Channel(fs, seed=2024, backend='hip', max_samples=B * step + ov, max_source=batch.total)
    chan.set_source(batch)
    frames = [chan.frame(starts[f], int(batch.sample_off[f]), length, 1.0, doppler[f], rate[f], 0.3 * f) for f in range(2)]
    sigma = chan.sigma_for(15.0, power=1.0)
    src = LoopbackSource(chan, frames, N, ov, B, nwin, sigma=sigma, keep_host=True)
    res, packets = run.run_device_stream(src, decoder=Decoder({}, p))
    run.close()
    assert len(res) == B * nwin and [d['count'] for d in res] == list(range(B * nwin))
    assert len(packets) == 2
    for pk, pl in zip(packets, payloads):
        data, crc_err, _ = pk.getBinaryData()
        assert pk.packetLen == 42 and not crc_err and np.array_equal(data[:-2], pl)
    for f in range(2):
        mid = starts[f] + length // 2
        blk = min(mid // step, B * nwin - 1)                       # the block that holds the frame's middle
        want = doppler[f] + rate[f] * dur / 2
        print(f"frame {f}: block {blk} reports {res[blk]['doppler']:.1f} Hz, mid-frame Doppler {want:.1f} Hz, bin spacing {spacing:.1f} Hz")
        assert abs(res[blk]['doppler'] - want) <= spacing

    # the same windows, copied to the host as they were rendered, through the host-fed loop: window 0 without the muted overlap
    # the loop starts from, the others without the overlap they share with the one before
    wins = src.host_windows
    assert len(wins) == nwin and np.all(wins[0][:ov] == 0) and np.array_equal(wins[0][-ov:], wins[1][:ov])
    tx.close()
    chan.close()
    run2 = DemodulatorRunner(conf, p, 'UHF-H')
    res2, packets2 = run2.run_stream([w[ov:] for w in wins], decoder=Decoder({}, p), blocks_per_call=B)
    run2.close()
    assert len(res2) == len(res) and len(packets2) == 2
    for a, b in zip(res, res2):
        assert a['count'] == b['count'] and np.array_equal(a['data'], b['data']), a['count']
        # (bit patterns: a block of noise alone may report an SNR that is not a number, the same one on both ways)
        assert np.float64(a['doppler']).tobytes() == np.float64(b['doppler']).tobytes(), a['count']
        assert np.float64(a['SNR']).tobytes() == np.float64(b['SNR']).tobytes(), a['count']
    for a, b in zip(packets, packets2):
        assert np.array_equal(a.getBinaryData()[0], b.getBinaryData()[0]) and a.packetLen == b.packetLen
