#!/usr/bin/env python3
"""Rates of the device channeliser (csrc/channelize_kernels.hpp); the figures of profiles/channelizer.md.

  python tools/channelize_rate.py [--reps 20] [--warmup 3] [--log2 22] [--configs 1,4,65 8,16,128 ...] [--no-torch] [--only-kernel]

Per configuration (K, D, T) and sample format (cf32, sc16): one call on 2^22 wideband samples already in device memory, the
outputs left there.  A call is timed with the library's events around its kernel (mfb_channelizer_elapsed_ms): the median of
--reps calls after --warmup untimed ones.  Beside the rate, the two rooflines: the input bytes over the HBM peak, and
8 K M T flops (M outputs per channel) over the fp32 vector peak -- the peaks bench.py's roofline uses.  And a yardstick written
with the plumbing library alone, in the same process on the same shapes: a torch mix of the window per channel, then
torch.nn.functional.conv1d with stride D on the real and imaginary planes, timed with torch's events.
--only-kernel runs each configuration's calls and nothing else (for a counters-only profiler run).  One JSON line per figure.
Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd.channelizer import Channelizer  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (bench.py)
VALU_FP32_PEAK = 157.3e12  # FLOP/s (bench.py)
FS = 1.0e6


def device_input(rs, n, fmt):
    import torch
    if fmt == 'cf32':
        x = (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)
    else:
        x = rs.randint(-20000, 20000, (n, 2)).astype(np.int16)
    return x, torch.from_numpy(x).cuda()


def torch_yardstick(x_dev, taps, freqs, D, nout, first, reps, warmup):
    """Per channel: mix the window, then conv1d with stride D on the two planes.  Returns (median ms, outputs [K, nout] complex64)."""
    import torch
    T = len(taps)
    n = x_dev.numel()
    w = torch.from_numpy(taps[::-1].copy()).cuda().reshape(1, 1, T)
    pos = torch.arange(first, first + n, device='cuda', dtype=torch.float64)
    out = torch.empty((len(freqs), nout), dtype=torch.complex64, device='cuda')

    def run():
        for k, f in enumerate(freqs):
            ph = torch.remainder(pos * (-f / FS), 1.0) * (2 * np.pi)
            z = x_dev * torch.polar(torch.ones_like(ph), ph).to(torch.complex64)
            planes = torch.view_as_real(z).t().reshape(2, 1, n)
            y = torch.nn.functional.conv1d(planes, w, stride=D)
            out[k] = torch.complex(y[0, 0, :nout], y[1, 0, :nout])
    for _ in range(warmup):
        run()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--configs', nargs='+', default=['1,4,65', '8,16,128', '16,16,257', '8,64,1024'])
    ap.add_argument('--formats', nargs='+', default=['cf32', 'sc16'])
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--only-kernel', action='store_true')
    args = ap.parse_args()
    n = 1 << args.log2
    rs = np.random.RandomState(1)
    for spec in args.configs:
        K, D, T = (int(v) for v in spec.split(','))
        taps = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
        freqs = list(np.linspace(-0.4, 0.4, K) * FS) if K > 1 else [0.123 * FS]
        # outputs whose inputs all lie inside [0, n): the first one is ceil((T - 1) / D)
        out_base = -(-(T - 1) // D)
        nout = (n - 1) // D - out_base + 1
        for fmt in args.formats:
            x, x_dev = device_input(rs, n, fmt)
            cz = Channelizer(FS, D, taps, freqs, sample_format=fmt, sample_scale=2.0 ** -15, max_in=n, max_out=nout)
            first, need = cz.needed_input(out_base, nout)
            item = 8 if fmt == 'cf32' else 4
            src = (x_dev.data_ptr() + first * item, need)
            ms = []
            for i in range(args.warmup + args.reps):
                cz.process(first, src, out_base, nout, copy=False)
                if i >= args.warmup:
                    ms.append(cz.elapsed_ms())
            if args.only_kernel:
                cz.close()
                continue
            med = float(np.median(ms))
            flops = 8.0 * K * nout * T
            line = {'what': f'channelise K={K} D={D} T={T} {fmt}, 2^{args.log2} input samples on the device', 'tile': cz.info()[0],
                    'outputs_per_channel': nout, 'ms': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4),
                    'wideband_Msamples_per_s': round(n / med / 1e3, 1), 'TFLOP_per_s': round(flops / med / 1e9, 2),
                    'frac_of_fp32_vector_peak': round(flops / (med * 1e-3) / VALU_FP32_PEAK, 4),
                    'frac_of_hbm_peak_input_bytes': round(n * item / (med * 1e-3) / HBM_PEAK, 4),
                    'roofline_ms_flops': round(flops / VALU_FP32_PEAK * 1e3, 4), 'roofline_ms_hbm': round(n * item / HBM_PEAK * 1e3, 5)}
            if not args.no_torch and fmt == 'cf32':
                got = cz.process(first, src, out_base, nout, copy=True)
                tms, ty = torch_yardstick(x_dev[first:first + need], taps, freqs, D, nout, first, max(5, args.reps // 2), 2)
                scale = float(np.abs(got).max())
                line.update({'torch_mix_conv1d_ms': round(tms, 4), 'torch_wideband_Msamples_per_s': round(n / tms / 1e3, 1),
                             'speedup_over_torch': round(tms / med, 2),
                             'max_abs_difference_from_torch_over_max_abs': round(float(np.abs(got - ty).max()) / scale, 8)})
            print(json.dumps(line), flush=True)
            cz.close()


if __name__ == '__main__':
    main()
