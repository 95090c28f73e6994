#!/usr/bin/env python3
"""Record ``ref_configs.json``: what the reference's own configuration files (its ``config/benchmark/bench_*.json`` and
``config/CC11xx.json``, layered through "configBase") say, read with our ``load_config``, on every key that
tests/test_config_loader.py compares with the dictionaries our builders produce.

Test infrastructure, run by hand where a checkout of the reference (pyCuSDR) exists; the JSON it writes is committed and is
what the tests read.  Only the loaded values are stored, never the files themselves.

Usage:  python tests/golden/make_golden_configs.py PATH/TO/pyCuSDR      (writes tests/golden/ref_configs.json)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pycusdr_amd import config as cfg  # noqa: E402

BENCH = ['bench_GMSK', 'bench_FSK', 'bench_GFSK', 'bench_BPSK']
RX_KEYS = ['CUDA_settings', 'frequency_Hz', 'frequencyOffset_Hz', 'baud', 'samplesPerSym', 'doppCarrierSteps', 'Protocol',
           'radioBackend']


def record(ref_root):
    out = {}
    for name in BENCH:
        c = cfg.load_config(os.path.join(ref_root, 'config', 'benchmark', name + '.json'))
        out[name] = {
            'Main': {'protocols': {'UHF': c['Main']['protocols']['UHF']}, 'PacketLen': c['Main']['PacketLen'],
                     'RandSeed': c['Main']['RandSeed']},
            'Radios': {'rangeRateMax': c['Radios']['rangeRateMax'],
                       'Rx': {'UHF-H': {k: c['Radios']['Rx']['UHF-H'][k] for k in RX_KEYS}}},
            'GPU': {s: c['GPU'][s] for s in ('UHF', 'STX')},
        }
    c = cfg.load_config(os.path.join(ref_root, 'config', 'CC11xx.json'))
    out['CC11xx'] = {
        'Radios': {'rangeRateMax': c['Radios']['rangeRateMax'],
                   'Protocol': {k: c['Radios']['Protocol'][k] for k in ('rx_preamble', 'rx_sync_seq')},
                   'Rx': {n: {k: r[k] for k in ('frequency_Hz', 'frequencyOffset_Hz', 'baud', 'samplesPerSym', 'radioBackend')}
                          for n, r in c['Radios']['Rx'].items()}},
        'GPU': {'UHF': {'blockSize': c['GPU']['UHF']['blockSize']}},
    }
    return out


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'config')):
        raise SystemExit('usage: make_golden_configs.py PATH/TO/pyCuSDR  (a checkout of the reference with its config/ folder)')
    with open(os.path.join(HERE, 'ref_configs.json'), 'w') as f:
        json.dump(record(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write('\n')
