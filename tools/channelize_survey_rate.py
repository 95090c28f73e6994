#!/usr/bin/env python3
"""Rates of the survey of the raster (csrc/channelize_survey_kernels.hpp); the figures of profiles/channelizer_survey.md.

  python tools/channelize_survey_rate.py [--reps 20] [--warmup 3] [--log2 22] [--cell 256] [--configs 64,16,257 64,32,513 ...]
                                         [--only a|b|c]

Per configuration (M, D, T), all M bins selected, one call on 2^22 wideband complex64 samples already in device memory, timed with
the library's events (mfb_channelizer_elapsed_ms, which cover the survey's two launches): the median of --reps calls after --warmup
untimed ones, with the least and the most, of
  (a) a plain call that writes all M bins (the uniform kernel as it was),
  (b) a survey that writes nothing,
  (c) a survey that writes all M bins,
in the same process on the same input, over the same span of outputs (a multiple of the cell length).  Acceptance: (b) <= (a) and
(c) < (a) + (b).  --only runs one of the three and nothing else (for a counters-only profiler run).  One JSON line per
configuration.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pycusdr_amd.channelizer import UniformChannelizer  # noqa: E402

FS = 1.024e6


def stats(ms):
    return {'ms': round(float(np.median(ms)), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log2', type=int, default=22)
    ap.add_argument('--cell', type=int, default=256)
    ap.add_argument('--configs', nargs='+', default=['64,16,257', '64,32,513', '256,128,2049'])
    ap.add_argument('--only', choices=['a', 'b', 'c'])
    args = ap.parse_args()
    n, L = 1 << args.log2, args.cell
    rs = np.random.RandomState(1)
    x = (0.3 * (rs.standard_normal(n) + 1j * rs.standard_normal(n))).astype(np.complex64)
    x_dev = torch.from_numpy(x).cuda()
    for spec in args.configs:
        M, D, T = (int(v) for v in spec.split(','))
        taps = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
        # whole cells whose inputs all lie inside [0, n)
        first_cell = -(-(T - 1) // (D * L))
        ncells = ((n - 1) // D + 1) // L - first_cell
        nout = ncells * L
        uz = UniformChannelizer(FS, M, D, taps, max_in=n, max_out=nout)
        uz.set_survey(L)
        first, need = uz.needed_input_cells(first_cell, ncells)
        src = (x_dev.data_ptr() + first * 8, need)
        runs = {'a': lambda: uz.process(first, src, first_cell * L, nout, copy=False),
                'b': lambda: uz.survey(first, src, first_cell, ncells),
                'c': lambda: uz.survey(first, src, first_cell, ncells, write=True, copy=False)}
        if args.only:
            runs = {args.only: runs[args.only]}
        ms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, run in runs.items():                      # interleaved: a drift of the clocks falls on all three alike
                run()
                if i >= args.warmup:
                    ms[k].append(uz.elapsed_ms())
        info = uz.survey_info()
        frames = uz.info()[0]
        uz.close()
        if args.only:
            continue
        a, b, c = (stats(ms[k]) for k in 'abc')
        print(json.dumps({'what': f'survey M={M} D={D} T={T} L={L}, all bins, 2^{args.log2} cf32 input samples on the device',
                          'frames_per_workgroup': frames, 'survey_frames_per_workgroup': info[0], 'cells': ncells, 'outputs_per_bin': nout,
                          'a_plain_write_all': a, 'b_survey_only': b, 'c_survey_and_write': c,
                          'b_over_a': round(b['ms'] / a['ms'], 3), 'c_over_a': round(c['ms'] / a['ms'], 3),
                          'c_over_a_plus_b': round(c['ms'] / (a['ms'] + b['ms']), 3),
                          'bytes_in': n * 8, 'bytes_out': M * nout * 8, 'bytes_tables': ncells * (M * 4 + 4 + -(-M // 32) * 4)}), flush=True)


if __name__ == '__main__':
    main()
