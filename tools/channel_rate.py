#!/usr/bin/env python3
"""Rates of the device channel (csrc/channel_kernels.hpp) and of the loopback through it; the figures of profiles/channel.md.

  python tools/channel_rate.py [--reps 20] [--warmup 3] [--sizes 16 20 24] [--no-loopback] [--no-host]

Render rates: windows of 2^16, 2^20 and 2^24 samples, each with noise only, frames only, both, and both with an ADC, with the
output left on the device and copied to the host.  A call is timed with the host clock from mfb_channel_begin to the return of
mfb_channel_end, which waits for the device (the descriptors are packed before the clock starts); the median of --reps calls
after --warmup untimed ones.  Beside them
``signals.awgn`` plus the ``np.exp`` mix for the same window on this machine's CPU.

Loopback: ``LoopbackSource`` -> ``run_device_stream`` with the decoder on, at 2^15 x 64 bins x 32 blocks per call (bench GMSK) and
at the CC11xx geometry (2^17 x 64 x 8), against ``run_device_stream`` over windows rendered beforehand -- the receive chain alone.
One JSON line per figure.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd import config as cfg, signals as sg  # noqa: E402
from pycusdr_amd.channel import Channel, LoopbackSource, pack_frames  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def render_rates(args):
    rs = np.random.RandomState(1)
    L = 1 << 14
    src = np.exp(2j * np.pi * rs.uniform(0, 1, L)).astype(np.complex64)
    for lg in args.sizes:
        n = 1 << lg
        ch = Channel(1.0e6, seed=7, max_samples=n, max_source=L, max_frames=max(1, n // (L + 1000)) + 1)
        ch.set_source(src)
        # copies of the source with gaps of 1000 samples, every one on its own drifting carrier
        frames = [ch.frame(s, 0, L, 1.0, 1000.0 + i, 5.0e4, 0.1 * i) for i, s in enumerate(range(500, n - L, L + 1000))]
        if not frames:
            frames = [ch.frame(500, 0, min(L, n - 500), 1.0, 1000.0, 5.0e4)]
        frames = pack_frames(frames)        # packed before the clock starts, as modulate_rate.py packs its bits
        for label, fr, sigma, adc in (('noise only', frames[:0], 0.5, None), ('frames only', frames, 0.0, None), ('both', frames, 0.5, None),
                                      ('both with a 16-bit ADC', frames, 0.5, (16, 2.0 ** -12))):
            for where, copy in (('device', False), ('host', True)):
                ms, lo, hi = median_ms(lambda: ch.render(0, n, fr, sigma, adc=adc, copy=copy), args.reps, args.warmup)
                print(json.dumps({'what': f'render 2^{lg}, {label}, output on {where}', 'samples': n, 'frames': len(fr), 'ms': round(ms, 4),
                                  'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'Msamples_per_s': round(n / ms / 1e3, 1),
                                  'GB_per_s_stored': round(8 * n / ms / 1e6, 2)}), flush=True)
        ch.close()
        if not args.no_host and lg <= 20:
            sig = np.zeros(n, dtype=np.complex128)
            sig[500:500 + L] = src
            rng = np.random.RandomState(2)

            def host():
                return sg.awgn(sig * np.exp(1j * 2 * np.pi * 0.01 * np.arange(n)), 10.0, rng=rng).astype(np.complex64)
            ms, _, _ = median_ms(host, max(3, args.reps // 4), 1)
            print(json.dumps({'what': f'signals.awgn + np.exp mix 2^{lg}, CPU', 'samples': n, 'ms': round(ms, 3),
                              'Msamples_per_s': round(n / ms / 1e3, 2)}), flush=True)


class Prerendered:
    """The windows of a LoopbackSource rendered once, each into device memory of its own (channels of their own), and handed out
    again: ``run_device_stream`` on them is the receive chain alone."""

    def __init__(self, make_source, nwindows):
        self.items = []
        for w in range(nwindows):
            src = make_source()
            ptr, _ = src.render(w)
            self.items.append((src, ptr, src.B))

    def __iter__(self):
        return iter([(ptr, nb) for _, ptr, nb in self.items])

    def close(self):
        for src, _, _ in self.items:
            src.channel.close()


def loopback(args):
    from pycusdr_amd.decoder import Decoder
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.modulator import Modulator
    from pycusdr_amd.protocol import loadProtocol
    for name, bs, B, nwin in (('bench GMSK 2^15 x 64 x 32', 15, 32, 12), ('CC11xx 2^17 x 64 x 8', 17, 8, 12)):
        if name.startswith('bench'):
            conf = cfg.bench_config('bench_GMSK', blockSize=bs, doppCarrierSteps=64)
            proto = loadProtocol('bench_GMSK')(conf=conf)
            bits = [sg.packetData()]
        else:
            conf = cfg.cc11xx_config(blockSize=bs, doppCarrierSteps=64, samplesPerSym=128)
            proto = loadProtocol('CC11xx')(conf=conf)
            proto.CRC_CHECK = 'framer'
            bits = None
        radio = conf['Radios']['Rx']['UHF-H']
        fs = float(radio['baud'] * radio['samplesPerSym'])
        tx = Modulator(conf, radio, proto, backend='hip')
        batch = tx.modulate_device(bits if bits is not None else [tx.encodeAndFrame(np.arange(200, dtype=np.uint8))])
        run = DemodulatorRunner(conf, proto, 'UHF-H')
        N, ov = run.blockSize, run.overlap
        count = B * (N - ov) + ov
        total = nwin * B * (N - ov)
        period = batch.total + 20000

        def make_source():
            ch = Channel(fs, seed=11, max_samples=count, max_source=batch.total, max_frames=total // period + 1)
            ch.set_source(batch)
            frames = [ch.frame(s, 0, batch.total, 1.0, 500.0, 100.0) for s in range(ov + 10000, total - batch.total, period)]
            return LoopbackSource(ch, frames, N, ov, B, nwin, sigma=ch.sigma_for(14.0))
        dec = Decoder(conf, proto)
        dec.prepare()
        live = make_source()
        pre = Prerendered(make_source, nwin)
        for label, windows in (('loopback (render + receive)', live), ('receive alone (windows rendered beforehand)', pre)):
            rates, npk = [], 0
            for rep in range(args.loop_reps + 1):
                t0 = time.perf_counter()
                res, packets = run.run_device_stream(windows, decoder=dec)
                dt = time.perf_counter() - t0
                if rep:              # the first pass is untimed
                    rates.append(total / dt / 1e6)
                npk = len(packets)
            print(json.dumps({'what': f'{name}: {label}', 'samples': total, 'blocks': len(res), 'packets': npk,
                              'Msamples_per_s_median': round(float(np.median(rates)), 1), 'min': round(min(rates), 1),
                              'max': round(max(rates), 1)}), flush=True)
        pre.close()
        live.channel.close()
        run.close()
        tx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--loop-reps', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[16, 20, 24])
    ap.add_argument('--no-loopback', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    render_rates(args)
    if not args.no_loopback:
        loopback(args)


if __name__ == '__main__':
    main()
