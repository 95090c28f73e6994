"""``Modulator(backend='hip')``: against the fixtures recorded from the reference, against the 'host' back end, and looped back
through the receiver."""
import os

import numpy as np
import pytest

import modulator_model as mm
from pycusdr_amd import config as cfg, signals as sg
from pycusdr_amd.decoder import Decoder
from pycusdr_amd.modulator import Modulator
from pycusdr_amd.protocol import loadProtocol
from test_modulator_host import comp_dist, make_modulator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_goldens_modulator.npz'), allow_pickle=False)
    return {k.replace('__', '/'): z[k] for k in z.files}


def test_hip_backend_against_every_golden(gold):
    for mod in ('FSK', 'GMSK'):
        for i in range(int(gold[f'short/{mod}/count'])):
            p = f'short/{mod}/{i}/'
            m = make_modulator(gold, mod, int(gold[p + 'sps']), 'hip')
            m.pad_len = m.min_len = 0
            sig = m.modulate(gold[p + 'bits'])
            m.close()
            assert sig.dtype == np.complex64 and len(sig) == len(gold[p + 'ref'])
            d = comp_dist(sig, gold[p + 'ref'])
            print(f'{p} distance {d:.3e} (model to reference {float(gold[p + "dist"]):.3e})')
            assert d <= mm.BOUND + float(gold[p + 'dist']), (p, d)
        p = f'whole/{mod}/'
        m = make_modulator(gold, mod, 16, 'hip')
        sig = m.modulate(gold[p + 'bits'])
        m.close()
        assert sig.dtype == np.complex64 and len(sig) == len(gold[p + 'out'])
        d = comp_dist(sig, gold[p + 'out'])
        print(f'{p} distance {d:.3e}')
        assert d <= mm.BOUND + float(gold[p + 'dist'])


def test_hip_and_host_give_the_same_words(gold):
    rs = np.random.RandomState(11)
    for mod, sps in (('FSK', 16), ('GMSK', 16), ('GMSK', 5), ('FSK', 128)):
        hip, host = make_modulator(gold, mod, sps, 'hip'), make_modulator(gold, mod, sps, 'host')
        frames = [rs.randint(0, 2, n) for n in (2, 65, 300, 1025)]
        rates = [0.0, -7000.0, 3.5, 6100.0]
        a = hip.modulate_batch(frames, rangerates=rates)
        b = host.modulate_batch(frames, rangerates=rates)
        wa, wb = hip.phase_words(), host.phase_words()
        for f in range(len(frames)):
            assert np.array_equal(wa[f], wb[f]), (mod, sps, f)
            assert len(a[f]) == len(b[f]) and comp_dist(a[f], b[f]) <= 2 * mm.BOUND
            pre, _ = mm.layout(len(frames[f]) * sps, 4096, 16384)
            assert a[f][:pre + 4096].tobytes() == b[f][:pre + 4096].tobytes() and a[f][-4096:].tobytes() == b[f][-4096:].tobytes()
        hip.close()


def test_loopback_cc11xx_with_doppler_and_offset():
    """The geometry of test_cc11xx_frame_received_and_crc_ok; the frame comes from the device modulator, pre-compensated with a
    range rate, and carries the radio's IF offset."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, sps = 17, 128
    conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=sps)
    p = loadProtocol('CC11xx')(conf=conf)
    p.CRC_CHECK = 'framer'
    radio = conf['Radios']['Rx']['UHF-H']
    tx = Modulator(conf, radio, p, backend='hip')
    rangerate = 6100.0
    tx.set_rangerate(rangerate)
    payload = np.arange(1, 41, dtype=np.uint8)
    frame = tx.encodeAndModulate(payload)
    tx.close()
    assert frame.dtype == np.complex64 and len(frame) == (10 + 4 + 1 + 40 + 2) * 8 * sps + 8192
    sig = np.concatenate((np.zeros(9000), frame, np.zeros(7 * (1 << bs))))
    sig = sg.awgn(sig, 15.0, rng=np.random.RandomState(2)).astype(np.complex64)
    run = DemodulatorRunner(conf, p, 'UHF-H')
    step = (1 << bs) - (1 << 10)
    res, packets = run.run([sig[i * step:(i + 1) * step] for i in range(4)], decoder=Decoder({}, p))
    spacing = float(np.abs(np.diff(run.demod.doppHzLUT)).max())
    run.close()
    assert len(packets) == 1
    data, crc_err, _ = packets[0].getBinaryData()
    assert packets[0].packetLen == 42 and not crc_err and np.array_equal(data[:-2], payload)
    want = rangerate / 3e8 * radio['frequency_Hz']
    print(f"doppler reported {res[0]['doppler']:.1f} Hz, sent {want:.1f} Hz, bin spacing {spacing:.1f} Hz")
    assert abs(res[0]['doppler'] - want) <= spacing and abs(res[0]['spSymEst'] - 128) < 1


def test_loopback_bench_gmsk_hip_equals_host():
    """The bench GMSK packet at 2^15 x 32 bins: the receiver returns the same bits for the device-modulated frame as for the
    host-modulated one.  No error count is asserted: the receiver's filters come from another GMSK generator than the LUT's."""
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    bs, ov = 15, 1 << 10
    N = 1 << bs
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
    p = loadProtocol('bench_GMSK')(conf=conf)
    radio = conf['Radios']['Rx']['UHF-H']
    bits = sg.packetData()
    noise = (1e-8 * (np.random.RandomState(3).randn(16384) + 1j * np.random.RandomState(4).randn(16384))).astype(np.complex64)
    got = {}
    for backend in ('hip', 'host'):
        tx = Modulator(conf, radio, p, backend=backend, noise=noise)
        frame = tx.modulate(bits)
        words = tx.phase_words()[0]
        tx.close()
        sig = sg.awgn(np.concatenate((np.zeros(10000), frame, np.zeros(2 * N))), 12.0, rng=np.random.RandomState(4)).astype(np.complex64)
        step = N - ov
        run = DemodulatorRunner(conf, p, 'UHF-H')
        res, _ = run.run([sig[i * step:(i + 1) * step] for i in range(len(sig) // step)])
        run.close()
        got[backend] = (words, res)
    assert np.array_equal(got['hip'][0], got['host'][0])
    assert len(got['hip'][1]) == len(got['host'][1]) > 4
    nbits = 0
    for a, b in zip(got['hip'][1], got['host'][1]):
        assert np.array_equal(a['data'], b['data']), a['count']
        nbits += len(a['data'])
    assert nbits > 9000


def test_modulate_device_feeds_the_receiver_without_a_host_copy():
    """modulate_device leaves the batch on the device; the pointer of a frame goes to mfb_upload_device and gives the spectrum
    of the same samples uploaded from the host."""
    from pycusdr_amd.demodulator import UHF
    bs = 15
    N = 1 << bs
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
    p = loadProtocol('bench_GMSK')(conf=conf)
    tx = Modulator(conf, conf['Radios']['Rx']['UHF-H'], p, backend='hip')
    bits = sg.packetData()[:4000]
    host = tx.modulate_batch([bits[:100], bits], rangerates=[0.0, 1500.0])
    batch = tx.modulate_device([bits[:100], bits], rangerates=[0.0, 1500.0])
    assert batch.frame_len(1) == len(host[1]) >= 4096 + N
    demod = UHF.Demodulator(conf, p, 'UHF-H')
    demod.bank.upload_device(batch.frame_ptr(1, offset=4096))
    a = demod.bank.get_spectrum()
    demod.bank.upload(host[1][4096:4096 + N])
    b = demod.bank.get_spectrum()
    assert a.tobytes() == b.tobytes() and np.abs(a).max() > 0
    demod.close()
    tx.close()
