#!/usr/bin/env python3
"""Rates of the rational plans on the raster (csrc/channelize_uniform_rational_kernels.hpp); the figures of
profiles/channelizer_uniform_rational.md.

  python tools/channelize_uniform_rational_rate.py [--reps 20] [--warmup 3] [--log2 22] [--configs 64,8,125,16 ...]
                                                   [--format cf32|sc16] [--only rational|integer|two-stage ...]

Per configuration (M, U, D, selected bins), on 2^22 wideband samples already in device memory, the outputs left there, every call
timed with the library's events around its kernel (mfb_channelizer_elapsed_ms), the median of --reps after --warmup untimed ones:

  rational    one call of ``UniformChannelizer(M, D, design_taps(D, interp=U), interp=U)``.
  integer     the same-kernel yardstick: an integer uniform plan with the same M, D' = ceil(D / U) and ceil(T / U) taps -- the same
              multiply-adds per frame and about the same frames per input.
  two-stage   the route without rational plans on the raster: an integer uniform plan by D1 to an intermediate rate, then one
              rational ``Channelizer(freqs_hz=[0.0], interp=U)`` call per selected bin by U / (D / D1), fed the first stage's
              ``device_output`` pointer.  D1 is the largest divisor of D with D / D1 <= 64 and U < D / D1 that the raster allows.
              The sum of the calls' device times, and the wall time of the whole route between two device synchronisations.
              This part uses nothing that a library without the rational plans on the raster lacks.

One JSON line per figure.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd.channelizer import Channelizer, UniformChannelizer, design_taps  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (bench.py)
FS = 2.4e6


def span(cz, n):
    """The largest span of outputs whose inputs all lie inside [0, n): (out_base, nout, first, need)."""
    U, D = cz.interp, cz.decim
    out_base = -(-(cz.Tb - 1) * U // D)
    nout = min((n * U - 1) // D - out_base + 1, cz.max_out)
    while sum(cz.needed_input(out_base, nout)) > n:
        nout -= 1
    return (out_base, nout) + cz.needed_input(out_base, nout)


def timed(cz, src_ptr, item, n, reps, warmup):
    out_base, nout, first, need = span(cz, n)
    ms = []
    for i in range(warmup + reps):
        cz.process(first, (src_ptr + first * item, need), out_base, nout, copy=False)
        if i >= warmup:
            ms.append(cz.elapsed_ms())
    return ms, nout


def figures(ms):
    return {'ms': round(float(np.median(ms)), 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}


def two_stage(torch, x_ptr, item, n, M, U, D, bins, kw, reps, warmup):
    D1 = max((d for d in range(2, M + 1) if D % d == 0 and U < D // d <= 64), default=None)
    if D1 is None:
        return None
    D2 = D // D1
    s1 = UniformChannelizer(FS, M, D1, design_taps(D1), bins=bins, max_out=n // D1 + 1, **kw)
    ob1, n1, first1, need1 = span(s1, n)
    s2 = Channelizer(FS / D1, D2, design_taps(D2, interp=U), [0.0], max_in=n1, max_out=n1 * U // D2 + 1, interp=U)
    ob2, n2, first2, need2 = span(s2, n1)
    dev, wall = [], []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s1.process(first1, (x_ptr + first1 * item, need1), ob1, n1, copy=False, buffer=0)
        total = s1.elapsed_ms()
        for k in range(len(bins)):
            ptr, cnt = s1.device_output(0, k)
            assert cnt == n1
            s2.process(first2, (ptr + 8 * first2, need2), ob2, n2, copy=False)
            total += s2.elapsed_ms()
        torch.cuda.synchronize()
        if i >= warmup:
            dev.append(total)
            wall.append((time.perf_counter() - t0) * 1e3)
    s1.close()
    s2.close()
    return {'stage1': f'uniform D={D1} T={len(design_taps(D1))}', 'stage2': f'rational {U}/{D2} T={len(design_taps(D2, interp=U))} per bin',
            'calls': 1 + len(bins), 'outputs_per_bin': n2, 'device': figures(dev), 'wall': figures(wall),
            'intermediate_bytes': 2 * 8 * len(bins) * n1}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--configs', nargs='+', default=['64,8,125,1', '64,8,125,16', '64,8,125,64'])
    ap.add_argument('--format', default='cf32', choices=['cf32', 'sc16'])
    ap.add_argument('--only', nargs='+', default=['rational', 'integer', 'two-stage'], choices=['rational', 'integer', 'two-stage'])
    args = ap.parse_args()
    n = 1 << args.log2
    rs = np.random.RandomState(1)
    fmt = args.format
    item = 8 if fmt == 'cf32' else 4
    if fmt == 'cf32':
        x = (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)
    else:
        x = rs.randint(-20000, 20000, (n, 2)).astype(np.int16)
    x_dev = torch.from_numpy(x).cuda()
    kw = dict(sample_format=fmt, sample_scale=2.0 ** -15, max_in=n)
    for spec in args.configs:
        M, U, D, nsel = (int(v) for v in spec.split(','))
        bins = list(range(M)) if nsel == M else [int(b) for b in np.linspace(0, M - 1, nsel).round()]
        taps = design_taps(D, interp=U)
        T, Tb = len(taps), -(-len(taps) // U)
        what = f'M={M} U={U} D={D} T={T} (Tb={Tb}) {nsel} bins {fmt}, 2^{args.log2} input samples on the device'
        if 'rational' in args.only:
            uz = UniformChannelizer(FS, M, D, taps, bins=bins, max_out=n * U // D + 1, interp=U, **kw)
            ms, nout = timed(uz, x_dev.data_ptr(), item, n, args.reps, args.warmup)
            F = uz.info()[0]
            uz.close()
            nbytes = n * item + 8 * nsel * nout
            med = float(np.median(ms))
            print(json.dumps({'what': 'uniform rational ' + what, 'frames_per_workgroup': F, 'outputs_per_bin': nout, **figures(ms),
                              'wideband_Msamples_per_s': round(n / med / 1e3, 1), 'bytes_in_plus_out': nbytes,
                              'roofline_ms_hbm': round(nbytes / HBM_PEAK * 1e3, 5),
                              'frac_of_hbm_peak': round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}), flush=True)
        if 'integer' in args.only:
            Di = min(-(-D // U), M)
            ui = UniformChannelizer(FS, M, Di, design_taps(Di, 64)[:Tb], bins=bins, max_out=n // Di + 1, **kw)
            ms, nout = timed(ui, x_dev.data_ptr(), item, n, args.reps, args.warmup)
            F = ui.info()[0]
            ui.close()
            print(json.dumps({'what': f'uniform integer yardstick M={M} D={Di} T={Tb} {nsel} bins {fmt}', 'frames_per_workgroup': F,
                              'outputs_per_bin': nout, **figures(ms)}), flush=True)
        if 'two-stage' in args.only:
            got = two_stage(torch, x_dev.data_ptr(), item, n, M, U, D, bins, kw, args.reps, args.warmup)
            print(json.dumps({'what': 'two-stage route ' + what, **(got or {'skipped': 'no integer first stage divides D'})}), flush=True)


if __name__ == '__main__':
    main()
