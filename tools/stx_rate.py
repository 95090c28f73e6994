"""Receive-loop rate of the S-band (STX) back end at its production geometry -- blocks of 2^17 samples, overlap 2^11, peak
threshold scale 4.5 (pycusdr_amd/config.py) -- on a seeded GMSK packet stream with interference bursts: run_stream with the
peak clip on the host (the reference's __thresholdInput, DB:670-707) against the same stream with "HIP": {"device_clip": true}
(one block per call, overlapped, batches of the auto size, and the same batches with "stream_stages": false -- the bit lookup,
the block-overlap alignment and the clipped-peak tags on the host), and whether every non-timing result key and every packet
agree.  Prints one JSON line; `<leg>_stage_blocks` counts the blocks whose integer stages the device ran.
The clip kernels' time per block comes from a run of this script under `rocprofv3 --kernel-trace --stats` (k_clip_*).

    python tools/stx_rate.py [blocks] [bs]
"""
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TIMING = ('timestamp', 'time_ms', 'rate_ksps', 'rate_ksps_avg', 'latency_ms')


def _eq(u, v):
    u, v = np.asarray(u), np.asarray(v)
    if u.dtype.kind in 'fc' and v.dtype.kind in 'fc':
        return u.shape == v.shape and np.array_equal(u, v, equal_nan=True)
    return np.array_equal(u, v)


def main(nblocks=64, bs=17, ov_log2=11, scale=4.5):
    from pycusdr_amd import config as cfg, signals as sg
    from pycusdr_amd.decoder import Decoder
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.protocol import loadProtocol
    N, ov = 1 << bs, 1 << ov_log2
    conf = cfg.bench_config('bench_GMSK', blockSize=bs, overlap=ov_log2, doppCarrierSteps=8)
    conf['GPU']['UHF']['peakThresholdScale'] = scale
    conf['Radios']['Rx']['UHF-H']['radioBackend'] = 'STX'
    dconf = copy.deepcopy(conf)
    dconf['GPU']['UHF'].setdefault('HIP', {})['device_clip'] = True
    hconf = copy.deepcopy(dconf)
    hconf['GPU']['UHF']['HIP']['stream_stages'] = False
    p = loadProtocol('bench_GMSK')(conf=conf)
    sig = sg.s1_stream(nblocks, N, ov, 'GMSK', snr_db=12.0, seed=17)
    rng = np.random.default_rng(17)
    for p0 in rng.integers(ov, len(sig) - 64, 3 * nblocks):
        sig[p0:p0 + int(rng.integers(1, 40))] *= np.float32(rng.uniform(20, 2000))
    sig = sig[ov:]
    chunks = lambda: [sig[i:i + 65536] for i in range(0, len(sig), 65536)]
    out = {'blockSize': bs, 'overlap': ov, 'peakThresholdScale': scale, 'blocks': nblocks}
    res = {}
    legs = (('host_clip', conf, None), ('device_clip_b1', dconf, 1), ('device_clip_auto', dconf, None),
            ('device_clip_auto_host_stages', hconf, None))
    for name, c, B in legs:
        r = DemodulatorRunner(c, p, 'UHF-H')
        try:
            r.run_stream(chunks()[:8], decoder=Decoder(c, p), blocks_per_call=B)        # warm-up: graphs, buffers
            src = chunks()
            r.demod.stage_blocks = 0
            t0 = time.perf_counter()
            results, packets = r.run_stream(src, decoder=Decoder(c, p), blocks_per_call=B)
            dt = time.perf_counter() - t0
            if B is None and c is dconf:
                out['auto_blocks_per_call'] = r.auto_blocks_per_call()
        finally:
            r.close()
        out[name + '_msps'] = round(len(results) * (N - ov) / dt / 1e6, 1)
        out[name + '_stage_blocks'] = int(r.demod.stage_blocks)
        res[name] = (results, packets)
    ra, pa = res['host_clip']
    out['blocks_with_clipped_peaks'] = int(sum(1 for d in ra if (np.asarray(d['trust']) == 254).any()))
    same = True
    for name in ('device_clip_b1', 'device_clip_auto', 'device_clip_auto_host_stages'):
        rb, pb = res[name]
        same = same and len(ra) == len(rb) and len(pa) == len(pb) and all(np.array_equal(u.bits, v.bits) for u, v in zip(pa, pb))
        for x, y in zip(ra, rb):
            keys = set(x) - set(TIMING)
            same = same and keys == set(y) - set(TIMING) and all(_eq(x[k], y[k]) for k in keys)
    out['equal'] = bool(same)
    out['packets'] = len(pa)
    out['speedup_b1'] = round(out['device_clip_b1_msps'] / out['host_clip_msps'], 2)
    out['speedup_auto'] = round(out['device_clip_auto_msps'] / out['host_clip_msps'], 2)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main(*[int(a) for a in sys.argv[1:3]])
