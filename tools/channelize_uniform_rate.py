#!/usr/bin/env python3
"""Rates of the uniform polyphase channeliser (csrc/channelize_uniform_kernels.hpp); the figures of profiles/channelizer_uniform.md.

  python tools/channelize_uniform_rate.py [--reps 20] [--warmup 3] [--log2 22] [--configs 64,16,257,64 256,128,2049,16 ...]
                                          [--formats cf32] [--only-kernel]

Per configuration (M, D, T, selected bins) and sample format: one call on 2^22 wideband samples already in device memory, the
outputs left there.  A call is timed with the library's events around its kernel (mfb_channelizer_elapsed_ms): the median of
--reps calls after --warmup untimed ones.  Beside the time, the traffic the call cannot avoid -- the input read once, the
selected bins written once -- over it, as a fraction of the HBM peak bench.py's roofline uses.  And, in the same process on the
same input, the direct kernel (csrc/channelize_kernels.hpp) at the same (D, T) on as many of the selected bins as it takes, 16 at
the most, where its limits (D <= 64, T <= 1024) allow: the ratio of the two times is the acceptance figure of the profile.
--only-kernel runs each configuration's uniform calls and nothing else (for a counters-only profiler run).  One JSON line per
configuration.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd import channelizer as chz  # noqa: E402
from pycusdr_amd.channelizer import Channelizer, UniformChannelizer  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (bench.py)
FS = 1.024e6


def device_input(rs, n, fmt):
    import torch
    if fmt == 'cf32':
        x = (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)
    else:
        x = rs.randint(-20000, 20000, (n, 2)).astype(np.int16)
    return x, torch.from_numpy(x).cuda()


def timed(cz, first, src, out_base, nout, warmup, reps):
    ms = []
    for i in range(warmup + reps):
        cz.process(first, src, out_base, nout, copy=False)
        if i >= warmup:
            ms.append(cz.elapsed_ms())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--configs', nargs='+', default=['64,16,257,64', '64,32,513,64', '256,128,2049,256', '256,128,2049,16'])
    ap.add_argument('--formats', nargs='+', default=['cf32'])
    ap.add_argument('--only-kernel', action='store_true')
    args = ap.parse_args()
    n = 1 << args.log2
    rs = np.random.RandomState(1)
    for spec in args.configs:
        M, D, T, nsel = (int(v) for v in spec.split(','))
        taps = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
        bins = list(range(M)) if nsel == M else [int(b) for b in np.linspace(0, M - 1, nsel).round()]
        # outputs whose inputs all lie inside [0, n): the first one is ceil((T - 1) / D)
        out_base = -(-(T - 1) // D)
        nout = (n - 1) // D - out_base + 1
        for fmt in args.formats:
            x, x_dev = device_input(rs, n, fmt)
            item = 8 if fmt == 'cf32' else 4
            uz = UniformChannelizer(FS, M, D, taps, bins=bins, sample_format=fmt, sample_scale=2.0 ** -15, max_in=n, max_out=nout)
            first, need = uz.needed_input(out_base, nout)
            src = (x_dev.data_ptr() + first * item, need)
            ms = timed(uz, first, src, out_base, nout, args.warmup, args.reps)
            frames = uz.info()[0]
            uz.close()
            if args.only_kernel:
                continue
            med = float(np.median(ms))
            traffic = n * item + nsel * nout * 8
            line = {'what': f'uniform channeliser M={M} D={D} T={T} {nsel} bins {fmt}, 2^{args.log2} input samples on the device',
                    'frames_per_workgroup': frames, 'outputs_per_bin': nout, 'ms': round(med, 4), 'ms_min': round(min(ms), 4),
                    'ms_max': round(max(ms), 4), 'wideband_Msamples_per_s': round(n / med / 1e3, 1),
                    'bytes_in_plus_out': traffic, 'TB_per_s': round(traffic / (med * 1e-3) / 1e12, 3),
                    'frac_of_hbm_peak': round(traffic / (med * 1e-3) / HBM_PEAK, 4), 'roofline_ms_hbm': round(traffic / HBM_PEAK * 1e3, 5)}
            if D <= chz.MAX_DECIM and T <= chz.MAX_TAPS:
                k = min(nsel, chz.MAX_CHANNELS)
                b = np.array(bins[:k], dtype=np.int64)
                freqs = np.where(b >= M // 2, b - M, b) * (FS / M)
                cz = Channelizer(FS, D, taps, freqs, sample_format=fmt, sample_scale=2.0 ** -15, max_in=n, max_out=nout)
                dms = timed(cz, first, src, out_base, nout, args.warmup, args.reps)
                cz.close()
                dmed = float(np.median(dms))
                line.update({'direct_channels': k, 'direct_ms': round(dmed, 4), 'direct_ms_min': round(min(dms), 4),
                             'direct_ms_max': round(max(dms), 4), 'direct_over_uniform': round(dmed / med, 2)})
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
