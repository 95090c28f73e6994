"""Where does a create / use / close cycle leave memory behind?  Each stage runs `cycles` times; device free memory (hipMemGetInfo),
host RSS and open file descriptors are read before and after (after a few settling cycles).  Stages go from the bare runtime (streams,
events, page-locked and device buffers through ctypes on libamdhip64) over a bare handle to the runner of tools/soak.py.

    python tools/leak_probe.py [cycles=200] [stage,stage,...]
"""
import ctypes
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rss_mb():
    with open('/proc/self/statm') as f:
        return int(f.read().split()[1]) * os.sysconf('SC_PAGE_SIZE') / 2 ** 20


def main():
    import torch
    from pycusdr_amd import config as cfg, signals as sg
    from pycusdr_amd.decoder import Decoder
    from pycusdr_amd.demodulator import UHF
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.hostcpu import quiet_blas
    from pycusdr_amd.protocol import loadProtocol
    quiet_blas()
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    only = sys.argv[2].split(',') if len(sys.argv) > 2 else None
    torch.zeros(1, device='cuda')
    hip = ctypes.CDLL('libamdhip64.so')
    bs = 15
    N = 1 << bs
    sig, _ = sg.get_padded_packet('GMSK', 16, 153600)
    base = np.concatenate([sg.awgn(sig, 8.0, rng=np.random.RandomState(7)).astype(np.complex64) for _ in range(4)])
    step = N - 1024

    def stream(nblocks):
        need = nblocks * step + 1024
        s = np.tile(base, -(-need // len(base)))[:need]
        return (s[i:i + 16384] for i in range(0, len(s), 16384))

    def snap():
        torch.cuda.synchronize()
        free, _ = torch.cuda.mem_get_info()
        return free / 2 ** 20, rss_mb(), len(os.listdir('/proc/self/fd'))

    def hip_streams():
        s = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0
        assert hip.hipStreamDestroy(s) == 0

    def hip_priority_streams():
        s = ctypes.c_void_p()
        assert hip.hipStreamCreateWithPriority(ctypes.byref(s), 1, -1) == 0
        assert hip.hipStreamDestroy(s) == 0

    def hip_events():
        for _ in range(16):
            e = ctypes.c_void_p()
            assert hip.hipEventCreateWithFlags(ctypes.byref(e), 2) == 0
            assert hip.hipEventDestroy(e) == 0

    def hip_pinned():
        p = ctypes.c_void_p()
        assert hip.hipHostMalloc(ctypes.byref(p), ctypes.c_size_t(1 << 20), 0) == 0
        assert hip.hipHostFree(p) == 0

    def hip_device():
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(3 << 20)) == 0
        assert hip.hipFree(p) == 0

    conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
    proto = loadProtocol('bench_GMSK')(conf=conf)

    def handle_only():
        d = UHF.Demodulator(conf, proto, 'UHF-H')
        d.close()

    x0 = np.tile(base, 2)[:N].copy()

    def handle_search():
        d = UHF.Demodulator(conf, proto, 'UHF-H')
        d.bank.upload(x0)
        d.bank.find_carrier()
        d.close()

    def handle_blocks():
        d = UHF.Demodulator(conf, proto, 'UHF-H')
        for _ in range(4):          # the recorded graph of a block appears with its second use
            d.uploadAndFindCarrier(x0.copy())
            d.demodulate()
        d.close()

    def runner(bpc, decode=True, collect=False, blocks=12):
        def f():
            c2 = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=32)
            if bpc:
                c2['GPU']['UHF'].setdefault('HIP', {})['blocks_per_call'] = bpc
            run = DemodulatorRunner(c2, proto, 'UHF-H')
            dec = None
            if decode:
                dec = Decoder(c2, proto)
                dec.prepare()
            run.run_stream(stream(blocks), decoder=dec)
            run.close()
            del run, dec
            if collect:
                gc.collect()
        return f

    def decoder_only():
        dec = Decoder(conf, proto)
        dec.prepare()
        del dec

    def live():
        import collections
        names = ('MFBank', 'SyncFinder', 'Decoder', 'DemodulatorRunner', 'HostCopy', 'Demodulator')
        cnt = collections.Counter(type(o).__name__ for o in gc.get_objects() if type(o).__name__ in names)
        with open('/proc/self/status') as fh:
            thr = [ln.split()[1] for ln in fh if ln.startswith('Threads:')][0]
        return ', '.join(f'{k} {v}' for k, v in sorted(cnt.items())) + f'; threads {thr}'

    def handle_windows(nb):
        def f():
            d = UHF.Demodulator(conf, proto, 'UHF-H')
            d.bank.windows(nb, step)
            d.close()
        return f

    def batch_handle(stages_on, passes):
        def f():
            d = UHF.Demodulator(conf, proto, 'UHF-H')
            w = d.blockWindows(16)
            if stages_on:
                d.enableStreamStages()
                d.seedStreamStages()
            need = 12 * step + 1024
            w[0][:need] = np.tile(base, -(-need // len(base)))[:need]
            for _ in range(passes):
                d.beginBlocks(0, 12, source='window')
                d.waitBlocks(0)
            d.close()
        return f

    def host_copy():
        from pycusdr_amd.mfbank import HostCopy
        hc = HostCopy()
        dst = np.zeros(1 << 16, np.complex64)
        hc.submit(dst, 0, base[:4096])
        hc.drain()
        hc.close()

    def pinned_big():
        p = ctypes.c_void_p()
        assert hip.hipHostMalloc(ctypes.byref(p), ctypes.c_size_t(9 << 20), 0) == 0
        assert hip.hipHostFree(p) == 0

    def device_big():
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(40 << 20)) == 0
        assert hip.hipFree(p) == 0

    taps = np.zeros((2, N), np.complex64)
    taps[:, :32] = np.random.RandomState(0).standard_normal((2, 32))
    late_masks = np.conj(np.fft.fft(taps, axis=1)).astype(np.complex64)      # a short impulse response: the segment path, where batches run

    def late_allocations():
        """Everything a handle allocates after mfb_create, once per cycle (the cycle of tests/test_gpu_lifetime.py, at this probe's
        size): two streams with the clip on a batch, the spectrum mirror and its stream, the energy search, the span basis, the
        integer-sample staging -- then a sync finder and a combiner."""
        from pycusdr_amd.mfbank import Combiner, MFBank, SyncFinder
        b = MFBank(bs, 8, 2)
        b.set_filters(late_masks)
        b.set_shifts(list(range(8)))
        b.set_batch_overlap(True)
        b.set_peak_clip(4.5, 1024)
        w = b.windows(4, step)[0]
        w[:] = np.tile(base, -(-w.size // len(base)))[:w.size]
        b.begin_blocks(0, 4, 300, 200, 8, source='window')
        b.end_blocks_record(0)
        b.set_peak_clip(0)
        for _ in range(2):
            b.upload(x0)
            b.get_spectrum(0, 16)
        b.set_search_mode('energy')
        b.find_carrier()
        b.set_search_mode('transforms')
        b.set_search_basis('span')
        b.find_carrier()
        b.set_sample_format('sc16')
        b.input[:] = 1
        b.upload()
        b.close()
        bits = (np.arange(6000) % 3 == 0).astype(np.uint8)
        sf = SyncFinder([np.ones(16, np.int8)], [12], max_bits=1 << 12)
        sf.find(bits)
        sf.close()
        cmb = Combiner(max_bits=1 << 12, max_slaves=0)
        cmb.combine(bits[:4096], np.ones(4096, np.int8), [], 3.0, 16)
        cmb.close()

    small_taps = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    small_in = (np.arange(64) % 7 - 3 + 1j * (np.arange(64) % 5 - 2)).astype(np.complex64)
    small_bits = np.zeros(64, np.uint8)
    small_bits[20:36] = 1

    def side_handles():
        """The six side handles (csrc/stage_handle.hpp) at the smallest shapes each accepts -- those of tests/side_handles.py --:
        created, run once, destroyed."""
        from pycusdr_amd.channel import Channel
        from pycusdr_amd.channelizer import Channelizer, UniformChannelizer
        from pycusdr_amd.mfbank import Combiner, SyncFinder
        from pycusdr_amd.modulator.device import DeviceModulator
        from pycusdr_amd.synthesizer import UniformSynthesizer
        sf = SyncFinder([np.ones(16, np.int8)], [16], max_hits=4, max_bits=64)
        sf.find(small_bits)
        sf.close()
        cmb = Combiner(max_bits=64, max_slaves=0)
        cmb.combine(small_bits, np.full(64, 5, np.int8), [], 3.0, 16)
        cmb.close()
        mod = DeviceModulator(2, 4)
        mod.set_lut(0, np.array([[-0.3, -0.3], [0.3, 0.3]]))
        mod.begin([np.array([1, 0])])
        mod.end(copy=False)
        mod.close()
        ch = Channel(1.0, seed=5, max_samples=3, max_source=4, max_frames=1)
        ch.render(1, 3, sigma=1.0)
        ch.close()
        chz = Channelizer(1.0, 2, small_taps, [0.25], max_in=16, max_out=8)
        chz.process(0, small_in[:16], 0, 4)
        chz.close()
        chu = UniformChannelizer(1.0, 8, 2, small_taps, bins=[1], max_in=64, max_out=8)
        chu.process(0, small_in, 0, 4)
        chu.close()
        syn = UniformSynthesizer(1.0, 8, 2, small_taps, max_out=5, max_source=4, max_frames=1)
        syn.set_source(small_in[:4])
        syn.process(0, 5, [syn.placement(1, 0, 0, 4)])
        syn.close()

    stages = [('hip_streams', hip_streams), ('hip_priority_streams', hip_priority_streams), ('hip_events', hip_events),
              ('hip_pinned', hip_pinned), ('hip_device', hip_device), ('handle_only', handle_only), ('handle_search', handle_search),
              ('handle_blocks', handle_blocks), ('runner_b1', runner(1)), ('runner_b4', runner(4)), ('runner_auto', runner(0)),
              ('runner_b16', runner(16)), ('runner_b16_nodec', runner(16, decode=False)),
              ('runner_b16_gc', runner(16, collect=True)), ('runner_b16_48', runner(16, blocks=48)), ('decoder_only', decoder_only), ('runner_b32', runner(32)), ('handle_windows4', handle_windows(4)),
              ('handle_windows32', handle_windows(32)), ('batch_once', batch_handle(False, 1)), ('batch_x3', batch_handle(False, 3)),
              ('batch_stages_once', batch_handle(True, 1)), ('batch_stages_x3', batch_handle(True, 3)), ('host_copy', host_copy),
              ('pinned_big', pinned_big), ('device_big', device_big), ('late_allocations', late_allocations),
              ('side_handles', side_handles)]
    for name, f in stages:
        if only and name not in only:
            continue
        for _ in range(8):
            f()
        a = snap()
        for i in range(cycles):
            f()
            if cycles >= 1000 and (i + 1) % (cycles // 10) == 0:       # a long run: does it level off?
                m = snap()
                print(f'  {name} after {i + 1}: device {a[0] - m[0]:+.1f} MiB, rss {m[1] - a[1]:+.1f} MiB', flush=True)
        b = snap()
        print(f'  live: {live()}')
        print(f'{name:22s} per cycle: device {(a[0] - b[0]) / cycles:+.4f} MiB, rss {(b[1] - a[1]) / cycles:+.4f} MiB, fds {(b[2] - a[2]) / cycles:+.3f}',
              flush=True)


if __name__ == '__main__':
    main()
