#!/usr/bin/env python3
"""Rates and the sample error of the device modulator (csrc/mod_kernels.hpp); the figures of profiles/modulator.md.

  python tools/modulate_rate.py [--frames 64] [--bits 10000] [--sps 16] [--reps 20] [--warmup 3] [--no-sweep]

Per modulation: Msamples/s of a batch of --frames frames and of one frame per call, with the output left on the device
and copied to page-locked host memory; beside them the 'host' back end and the float64 formula of signals.modulateFSK on
this machine's CPU.  A call is timed with the host clock from mfb_modulator_begin to the return of mfb_modulator_end, which
waits for the device; the median of --reps calls after --warmup untimed ones.

The sweep: 2^24 phase words spread over the whole circle with varying low bits, every sample against exp(2 pi i w / 2^64) in
float64; the worst component error per octant in units of 2^-24 (the bound of the tests is 4).
One JSON line per figure.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd import signals as sg  # noqa: E402
from pycusdr_amd.modulator import modulators, phase  # noqa: E402
from pycusdr_amd.modulator.device import DeviceModulator  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def rates(args):
    rs = np.random.RandomState(1)
    nsamp = args.bits * args.sps
    for mod, cls in (('FSK', modulators.FSKmod), ('GMSK', modulators.GMSKmod)):
        m = cls(None, {'samplesPerSym': args.sps})
        frames = [rs.randint(0, 2, args.bits).astype(np.uint8) for _ in range(args.frames)]
        dphi = rs.uniform(-0.1, 0.1, args.frames)
        dev = DeviceModulator(args.frames * args.bits, args.frames * nsamp)
        dev.set_lut(m.kind, m.LUT)

        def call(packed, d, copy):
            dev.begin_packed(*packed, d)
            dev.end(copy=copy, pinned=True)
        for label, fr, d in (('batch', frames, dphi), ('single', frames[:1], dphi[:1])):
            packed = dev.pack(fr)
            for where, copy in (('device', False), ('pinned host', True)):
                ms, lo, hi = median_ms(lambda: call(packed, d, copy), args.reps, args.warmup)
                n = len(fr) * nsamp
                print(json.dumps({'what': f'{mod} {label}, output on {where}', 'frames': len(fr), 'samples': n, 'ms': round(ms, 4),
                                  'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'Msamples_per_s': round(n / ms / 1e3, 1),
                                  'GB_per_s_stored': round(8 * n / ms / 1e6, 2)}), flush=True)
        dev.close()
        ms, _, _ = median_ms(lambda: phase.words_to_iq(phase.phase_words(m.kind, m.LUT, frames[0], dphi[0])).astype(np.complex64),
                             max(3, args.reps // 4), 1)
        print(json.dumps({'what': f"{mod} 'host' back end, one frame, CPU", 'samples': nsamp, 'ms': round(ms, 3),
                          'Msamples_per_s': round(nsamp / ms / 1e3, 2)}), flush=True)
    ms, _, _ = median_ms(lambda: sg.modulateFSK(frames[0], args.sps), max(3, args.reps // 4), 1)
    print(json.dumps({'what': 'signals.modulateFSK (float64 cumsum, mod, exp), one frame, CPU', 'samples': nsamp, 'ms': round(ms, 3),
                      'Msamples_per_s': round(nsamp / ms / 1e3, 2)}), flush=True)


def sweep():
    """2^24 words: four frames of 4096 bits x 1024 samples, each a ramp once round the circle (2^-22 turns per sample) plus an
    odd fraction, from a different start."""
    sps, nbits = 1024, 4096
    dev = DeviceModulator(nbits, nbits * sps)
    worst = np.zeros(8)
    mag = 0.0
    total = 0
    for k, frac in enumerate((0.0, 0.3141592653589793, 0.5772156649015329, 0.7071067811865476)):
        inc = 2 * np.pi * (2.0 ** -22 + frac * 2.0 ** -44)
        dev.set_lut(phase.FSK, np.full((2, sps), inc))
        dev.begin([np.ones(nbits, np.uint8)], np.array([2 * np.pi * frac * 2.0 ** -30]))
        sig, _ = dev.end(pinned=True)
        w = dev.phase_words()
        ref = phase.words_to_iq(w)
        err = np.maximum(np.abs(sig.real - ref.real), np.abs(sig.imag - ref.imag))
        octant = (w >> np.uint64(61)).astype(np.int64)
        for o in range(8):
            if (octant == o).any():
                worst[o] = max(worst[o], err[octant == o].max())
        mag = max(mag, np.abs(np.abs(sig.astype(np.complex128)) - 1).max())
        total += len(w)
    dev.close()
    print(json.dumps({'what': 'sample error sweep', 'words': total, 'worst_component_error_in_2^-24_per_octant':
                      [round(float(x) * 2 ** 24, 3) for x in worst], 'worst': round(float(worst.max()) * 2 ** 24, 3),
                      'worst_magnitude_error_in_2^-24': round(float(mag) * 2 ** 24, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--bits', type=int, default=10000)
    ap.add_argument('--sps', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-sweep', action='store_true')
    args = ap.parse_args()
    rates(args)
    if not args.no_sweep:
        sweep()


if __name__ == '__main__':
    main()
