#!/usr/bin/env python3
"""Rates of the uniform polyphase synthesiser (csrc/synthesize_uniform_kernels.hpp); the figures of profiles/synthesizer.md.

  python tools/synthesize_rate.py [--reps 20] [--warmup 3] [--log2 22] [--configs 64,16,257 256,64,1025] [--occupied 1 16 all]
                                  [--no-torch] [--no-route] [--only-kernel]

Per configuration (M, I, T) and number of occupied bins: one call that makes 2^22 wide outputs from a source already in device
memory, one placement per occupied bin over the whole span, the outputs left on the device.  A call is timed with the library's
events around its kernel (mfb_synthesizer_elapsed_ms): the median of --reps calls after --warmup untimed ones.  Beside the time:
  * the store roofline: the outputs written once (and the source read once) over the HBM peak bench.py's roofline uses;
  * the share of transforms a workgroup repeats, (J - 1) / F with J = ceil(T / I);
  * torch on the same GPU: conv_transpose1d of the same taps with stride I on the streams' real and imaginary parts, then the mix
    to b fs / M and the sum over the bins, 16 bins at a time, timed with torch's events;
  * the route that exists without the synthesiser: Modulator at the wide rate (I times the samples per symbol) and one Channel
    render of the same span with the frames on one bin's carrier -- per occupied bin, since a Channel's frames do not overlap in
    time, so n bins cost n times that (and a sum); wall clock around the synchronous calls.
--only-kernel runs the synthesiser's calls and nothing else (for a counters-only profiler run).  One JSON line per case.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd.synthesizer import UniformSynthesizer  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (bench.py)
FS = 1.024e6


def torch_route(x_dev, bins, M, I, taps, n, reps):
    """ms per call, median: the streams x_dev [nb, L] complex64 -> n wide samples"""
    import torch
    w = torch.from_numpy(taps.copy()).cuda().reshape(1, 1, -1)
    pos = torch.arange(n, device='cuda', dtype=torch.int64)
    ms = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = torch.zeros(n, dtype=torch.complex64, device='cuda')
        for c in range(0, len(bins), 16):
            b = torch.tensor(bins[c:c + 16], device='cuda', dtype=torch.int64)
            xs = torch.view_as_real(x_dev[c:c + 16]).permute(0, 2, 1).reshape(1, -1, x_dev.shape[1])      # [1, 2 k, L]
            y = torch.nn.functional.conv_transpose1d(xs, w.expand(xs.shape[1], 1, -1).contiguous(), stride=I, groups=xs.shape[1])[0, :, :n]
            y = torch.view_as_complex(y.reshape(len(b), 2, n).permute(0, 2, 1).contiguous())
            ph = (b[:, None] * pos[None, :]) % M
            out += (y * torch.polar(torch.ones_like(ph, dtype=torch.float32), ph.to(torch.float32) * (2 * np.pi / M))).sum(0)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms[1:]))


def existing_route(M, I, n, reps):
    """(modulator ms, channel ms), medians of wall clock: CC11xx frames at I times 16 samples per symbol that fill n wide
    samples, then one render of the n samples with them on the carrier of bin 1"""
    from pycusdr_amd import config as cfg
    from pycusdr_amd.channel import Channel
    from pycusdr_amd.modulator import Modulator
    from pycusdr_amd.protocol import loadProtocol
    conf = cfg.cc11xx_config(blockSize=17, doppCarrierSteps=64, samplesPerSym=16 * I)
    p = loadProtocol('CC11xx')(conf=conf)
    tx = Modulator(conf, conf['Radios']['Rx']['UHF-H'], p, backend='hip')
    tx.set_rangerate(0.0)
    one = tx.encodeAndFrame(np.arange(1, 41, dtype=np.uint8))
    length = (10 + 4 + 1 + 40 + 2) * 8 * 16 * I + 8192
    nframes = max(1, n // length)
    mod_ms, chan_ms = [], []
    chan = None
    for _ in range(reps + 1):
        t = time.perf_counter()
        batch = tx.modulate_device([one] * nframes)
        mod_ms.append((time.perf_counter() - t) * 1e3)
        if chan is None:
            chan = Channel(FS, seed=1, backend='hip', max_samples=n, max_source=batch.total, max_frames=nframes)
        chan.set_source(batch)
        frames = [chan.frame(f * length, int(batch.sample_off[f]), batch.frame_len(f), 1.0, FS / M) for f in range(nframes)]
        t = time.perf_counter()
        chan.render(0, n, frames, sigma=0.0, copy=False)
        chan_ms.append((time.perf_counter() - t) * 1e3)
    chan.close()
    tx.close()
    return float(np.median(mod_ms[1:])), float(np.median(chan_ms[1:])), nframes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--configs', nargs='+', default=['64,16,257', '256,64,1025'])
    ap.add_argument('--occupied', nargs='+', default=['1', '16', 'all'])
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--no-route', action='store_true')
    ap.add_argument('--only-kernel', action='store_true')
    args = ap.parse_args()
    import torch
    n = 1 << args.log2
    rs = np.random.RandomState(1)
    for spec in args.configs:
        M, I, T = (int(v) for v in spec.split(','))
        taps = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
        L = n // I
        route = None
        for occ in args.occupied:
            nb = M if occ == 'all' else int(occ)
            bins = list(range(M)) if nb == M else [int(b) for b in np.linspace(0, M - 1, nb).round()]
            x = (0.3 * (rs.standard_normal((nb, L)) + 1j * rs.standard_normal((nb, L)))).astype(np.complex64)
            x_dev = torch.from_numpy(x).cuda()
            s = UniformSynthesizer(FS, M, I, taps, max_out=n, max_frames=max(nb, 1))
            s.set_source((x_dev.data_ptr(), x_dev.numel()))
            pl = [s.placement(b, 0, k * L, L) for k, b in enumerate(bins)]
            ms = []
            for i in range(args.warmup + args.reps):
                s.process(0, n, pl, copy=False)
                if i >= args.warmup:
                    ms.append(s.elapsed_ms())
            F, R = s.info()
            s.close()
            if args.only_kernel:
                continue
            med = float(np.median(ms))
            traffic = n * 8 + nb * L * 8
            line = {'what': f'synthesiser M={M} I={I} T={T}, {nb} bins occupied, 2^{args.log2} wide outputs, source on the device',
                    'frames_per_workgroup': F, 'rows': R, 'repeated_transform_share': round((R - F) / F, 3), 'ms': round(med, 4),
                    'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'wide_Msamples_per_s': round(n / med / 1e3, 1),
                    'bytes_out_plus_source': traffic, 'frac_of_hbm_peak': round(traffic / (med * 1e-3) / HBM_PEAK, 4),
                    'roofline_ms_hbm': round(traffic / HBM_PEAK * 1e3, 5)}
            if not args.no_torch:
                tms = torch_route(x_dev, bins, M, I, taps, n, max(2, args.reps // 5))
                line.update({'torch_conv_transpose_mix_ms': round(tms, 3), 'torch_over_synthesiser': round(tms / med, 1)})
            if not args.no_route:
                if route is None:
                    route = existing_route(M, I, n, max(2, args.reps // 5))
                line.update({'modulator_wide_ms_per_bin': round(route[0], 3), 'channel_render_ms_per_bin': round(route[1], 3),
                             'wide_frames': route[2], 'existing_route_ms': round(nb * (route[0] + route[1]), 3),
                             'existing_route_over_synthesiser': round(nb * (route[0] + route[1]) / med, 1)})
            print(json.dumps(line), flush=True)
            del x_dev


if __name__ == '__main__':
    main()
