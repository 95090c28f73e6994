"""Child of tests/test_gpu_wrap_mfma.py and tests/test_gpu_wrap_sweep.py: the doppSum tables of a set of adversarial blocks in THIS
process's form of the 256-point search (MFB_SEG_WRAP_MFMA in the environment is read once per process).  Writes an .npz with, per input, the scores, the block's
spectrum (for the oracle) and the pick; with ``span`` also the scores and picks of the span basis on the same handle.
usage: wrap_child.py <protocol> <log2N> <D> <out.npz> [span]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pycusdr_amd import config as cfg, signals as sg                                  # noqa: E402
from pycusdr_amd.demodulator.demodulator_base import doppler_bin_table                 # noqa: E402
from pycusdr_amd.mfbank import MFBank                                                  # noqa: E402
from pycusdr_amd.protocol import loadProtocol                                          # noqa: E402


def inputs(N, shifts, V):
    """name -> complex64 block: a stream, full-scale bursts shorter than a segment on a -60 dB floor at several phases of the wrap
    window, pure tones on a bin and between two bins, a block that is zero except for one segment, and a peak-clipped stream."""
    rs = np.random.RandomState(7)
    out = {}
    out['stream'] = sg.s1_stream(1, N, 1 << 10, 'GMSK', snr_db=8.0, seed=41)[:N]
    floor = 1e-3 * (rs.standard_normal(N) + 1j * rs.standard_normal(N)) / np.sqrt(2)
    seg0 = 37 * V                                         # a segment start; its wrap window is [seg0 - 47, seg0 + 48)
    for ph in (-60, -40, -20, 0, 20, 40):
        x = floor.copy()
        b0 = seg0 + ph
        x[b0:b0 + 24] += np.exp(2j * np.pi * rs.random_sample(24))
        out[f'burst{ph:+d}'] = x
    n = np.arange(N)
    s_on = int(shifts[len(shifts) // 3])
    out['tone_on_bin'] = np.exp(2j * np.pi * s_on * n / N) + floor
    s_mid = 0.5 * (int(shifts[len(shifts) // 2]) + int(shifts[len(shifts) // 2 + 1]))
    out['tone_between_bins'] = np.exp(2j * np.pi * s_mid * n / N) + floor
    x = np.zeros(N, dtype=np.complex128)
    x[seg0:seg0 + 256] = rs.standard_normal(256) + 1j * rs.standard_normal(256)
    out['one_segment'] = x
    x = out['stream'].astype(np.complex128) * 3.0
    x[5000:5400] += 40.0 * np.exp(2j * np.pi * rs.random_sample(400))             # an interference burst
    mag = np.abs(x)
    lim = 4.0 * mag.mean()
    out['clipped'] = np.where(mag > lim, x * (lim / np.maximum(mag, 1e-30)), x)
    return {k: np.asarray(v, dtype=np.complex64) for k, v in out.items()}


def setup(name, log2N, D):
    """(handle with the protocol's bank and bin table, masks, shifts)"""
    N = 1 << log2N
    conf, sps, ms = cfg.bench_config(name, blockSize=log2N, doppCarrierSteps=D), 16, (5 if name == 'bench_BPSK' else 3)
    _, _, shifts, _ = doppler_bin_table(conf['Radios']['Rx']['UHF-H'], conf['Radios']['rangeRateMax'], N)
    M, masks = loadProtocol(name)(conf=conf).get_filter(N, sps, ms)
    bank = MFBank(log2N, D, M)
    bank.set_filters(masks)
    bank.set_shifts(shifts)
    return bank, masks, shifts


def main(name, log2N, D, out, span=False):
    bank, _, shifts = setup(name, log2N, D)
    V = bank.get_search_path()['valid_per_segment']
    res = {'shifts': np.asarray(shifts), 'filter_side': int(bank.get_search_info()['filter_side']), 'log2L': bank.get_search_path()['log2L'],
           'taps': bank.get_search_path()['taps'], 'rows': bank.get_search_basis()[1]}
    for k, x in inputs(1 << log2N, shifts, V).items():
        bank.upload(x)
        pick = bank.find_carrier()
        res[f'scores_{k}'] = bank.get_scores()
        res[f'X_{k}'] = bank.get_spectrum()
        res[f'pick_{k}'] = np.asarray(pick, dtype=np.float64)
    if span:                  # ... and once more with the span basis on the same handle
        bank.set_search_basis('span')
        res['span_rows'] = bank.get_search_basis()[1]
        res['span_filter_side'] = int(bank.get_search_info()['filter_side'])
        for k, x in inputs(1 << log2N, shifts, V).items():
            bank.upload(x)
            res[f'spanpick_{k}'] = np.asarray(bank.find_carrier(), dtype=np.float64)
            res[f'spanscores_{k}'] = bank.get_scores()
    np.savez(out, **res)
    bank.close()


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], span=len(sys.argv) > 5 and sys.argv[5] == 'span')
