#!/usr/bin/env python3
"""Soft combiner: time per call of the hip back end (mfb_combiner_*, popcount correlation + vote on the device) and of the
host back end (numpy FFT correlation + numpy vote) for 2 and 3 workers -- one master and 1 or 2 slaves -- with slave buffers
of n = 4 096, 58 834 and 2^18 bits and n / 2 new master bits.  Both back ends run the same call and must agree; wall time
per call, copies and the host's re-check of the decisions included.  One JSON line per case.

Usage:  python tools/combine_rate.py [--calls 20] [--device 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case(rs, n, workers):
    Lm = n // 2
    base = rs.randint(0, 2, n + 4096).astype(np.int8)
    trust = lambda k: rs.randint(-3, 4, k).astype(np.int8)      # noqa: E731
    m = base[1000:1000 + Lm] ^ (rs.random_sample(Lm) < 0.02)
    slaves = []
    for i in range(workers - 1):
        off = 137 * (i + 1)
        slaves.append((base[1000 - off:1000 - off + n] ^ (rs.random_sample(n) < 0.03), trust(n)))
    return m.astype(np.int8), trust(Lm), slaves


def per_call(f, calls):
    f()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from pycusdr_amd import softCombiner as sc
    conf = {'SoftCombiner': {'workerDataRequestThreshold': 3, 'minProcessingLength': 1000, 'workerDataTimeout': 3.5,
                             'varianceMultiplier': 15.0, 'masterVoteWeight': 1.2}}
    rs = np.random.RandomState(1)
    hip = sc.SoftCombiner(conf, backend='hip', device=a.device)
    host = sc.SoftCombiner(conf, backend='host')
    for n in (4096, 58834, 1 << 18):
        for workers in (2, 3):
            m, t, slaves = case(rs, n, workers)
            rh, rc = hip.combine(m, t, slaves), host.combine(m, t, slaves)
            same = rh['status'] == rc['status'] and rh['matched'] == rc['matched'] and np.array_equal(rh['bits'], rc['bits']) and \
                np.array_equal(rh['trust'], rc['trust']) and all(np.array_equal(x['val'], y['val']) for x, y in zip(rh['slaves'], rc['slaves']))
            hip_ms = per_call(lambda: hip.combine(m, t, slaves), a.calls)
            host_ms = per_call(lambda: host.combine(m, t, slaves), max(3, a.calls // 4))
            print(json.dumps({'n': n, 'workers': workers, 'master_bits': len(m), 'matched': rh['matched'], 'identical': bool(same),
                              'hip_ms_median': round(hip_ms[0], 4), 'hip_ms_min': round(hip_ms[1], 4),
                              'host_ms_median': round(host_ms[0], 4), 'host_ms_min': round(host_ms[1], 4),
                              'host_over_hip': round(host_ms[0] / hip_ms[0], 2), 'host_fallbacks': hip.host_fallbacks}), flush=True)
    hip.close()


if __name__ == '__main__':
    main()
