#!/usr/bin/env python3
"""Rates of the rational channeliser (csrc/channelize_rational_kernels.hpp); the figures of profiles/channelizer_rational.md.

  python tools/channelize_rational_rate.py [--reps 20] [--warmup 3] [--log2 22] [--configs 2,25,1 2,25,4 ...] [--format cf32]

Per configuration (U, D, K): ``design_taps(D, interp=U)`` (16 taps per phase, 15 at D = 64 to stay within 1024), K carriers, one call
on 2^22 wideband samples already in device memory, the outputs left there, timed with the library's events around its kernel
(mfb_channelizer_elapsed_ms): the median of --reps calls after --warmup untimed ones.  Beside it the integer kernel at the same D
and K with ``ceil(T / U)`` taps -- the same multiply-adds per output, 1 / U of the outputs per input -- and the HBM roofline for
the bytes moved (the input once, every output once).  One JSON line per figure.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd.channelizer import Channelizer, design_taps  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (bench.py)
VALU_FP32_PEAK = 157.3e12  # FLOP/s (bench.py)
FS = 1.0e6


def timed(cz, src_ptr, item, n, reps, warmup):
    """The largest span of outputs whose inputs all lie inside [0, n): (median ms, min, max, outputs per channel)."""
    U, D = cz.interp, cz.decim
    out_base = -(-(cz.Tb - 1) * U // D)
    nout = (n * U - 1) // D - out_base + 1
    while cz.needed_input(out_base, nout)[0] + cz.needed_input(out_base, nout)[1] > n:
        nout -= 1
    first, need = cz.needed_input(out_base, nout)
    ms = []
    for i in range(warmup + reps):
        cz.process(first, (src_ptr + first * item, need), out_base, nout, copy=False)
        if i >= warmup:
            ms.append(cz.elapsed_ms())
    return float(np.median(ms)), min(ms), max(ms), nout


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--configs', nargs='+', default=['2,25,1', '2,25,4', '2,25,16', '16,25,1', '16,25,4', '16,25,16', '31,64,16'])
    ap.add_argument('--format', default='cf32', choices=['cf32', 'sc16'])
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
    for spec in args.configs:
        U, D, K = (int(v) for v in spec.split(','))
        taps = design_taps(D, 16 if D * 16 + 1 <= 1024 else 15, interp=U)
        T = len(taps)
        freqs = list(np.linspace(-0.4, 0.4, K) * FS) if K > 1 else [0.123 * FS]
        kw = dict(sample_format=fmt, sample_scale=2.0 ** -15, max_in=n)
        cz = Channelizer(FS, D, taps, freqs, max_out=n * U // D + 1, interp=U, **kw)
        Tb = cz.Tb
        med, lo, hi, nout = timed(cz, x_dev.data_ptr(), item, n, args.reps, args.warmup)
        tile = cz.info()[0]
        cz.close()
        ci = Channelizer(FS, D, design_taps(D, 16)[:Tb], freqs, max_out=n // D + 1, **kw)
        imed, ilo, ihi, inout = timed(ci, x_dev.data_ptr(), item, n, args.reps, args.warmup)
        itile = ci.info()[0]
        ci.close()
        nbytes = n * item + 8 * K * nout
        flops = 8.0 * K * nout * Tb
        print(json.dumps({
            'what': f'resample U={U} D={D} T={T} (Tb={Tb}) K={K} {fmt}, 2^{args.log2} input samples on the device', 'tile': tile,
            'outputs_per_channel': nout, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4),
            'Msamples_per_s_in': round(n / med / 1e3, 1), 'Msamples_per_s_out_per_channel': round(nout / med / 1e3, 1),
            'Msamples_per_s_out_all_channels': round(K * nout / med / 1e3, 1), 'TFLOP_per_s': round(flops / med / 1e9, 2),
            'bytes_moved': nbytes, 'roofline_ms_hbm': round(nbytes / HBM_PEAK * 1e3, 5),
            'frac_of_hbm_peak': round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
            'frac_of_fp32_vector_peak': round(flops / (med * 1e-3) / VALU_FP32_PEAK, 4),
            'integer_kernel': {'D': D, 'T': Tb, 'K': K, 'tile': itile, 'outputs_per_channel': inout, 'ms': round(imed, 4),
                               'ms_min': round(ilo, 4), 'ms_max': round(ihi, 4), 'Msamples_per_s_in': round(n / imed / 1e3, 1),
                               'Msamples_per_s_out_all_channels': round(K * inout / imed / 1e3, 1),
                               'TFLOP_per_s': round(8.0 * K * inout * Tb / imed / 1e9, 2)}}), flush=True)


if __name__ == '__main__':
    main()
