"""Child of tests/test_gpu_wrap_split.py and tests/golden/make_golden_segw.py: the doppSum tables of the matrix-core search
(wrap_kernels.hpp, k_segw) at 2^18 samples in THIS process's rectangle (MFB_SEG_FSM_RECT in the environment is read once per process),
on the blocks that exercise the split of the segment windows.  Everything is regenerated from the seeds below; the shifts of a handle
of D bins are the first D of one table, so that a (block, shift) is the same search on every handle.
usage: split_child.py gmsk|t34 <D> <out.npz>

gmsk  the bench_GMSK bank: 8 filters of 48 taps
t34   8 filters of 34 seeded complex normal taps: window slots below offset -(T - 1) = -33 are zeroed by the kernel"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pycusdr_amd import config as cfg, signals as sg                                  # noqa: E402
from pycusdr_amd.demodulator.demodulator_base import doppler_bin_table                 # noqa: E402
from pycusdr_amd.protocol import loadProtocol                                          # noqa: E402

LOG2N = 18
N = 1 << LOG2N
V = 208                   # valid outputs of a 256-point segment at 34 ... 48 taps
DMAX = 130
SEG = 37                  # the segment the one-segment and the window inputs are about: [SEG V, SEG V + 256)
BANKS = {'gmsk': 48, 't34': 34}
SEEDS = {'stream': 41, 'one_segment': 13, 'steps': 17, 'window': 19, 't34': 5}
KINDS = ('stream', 'one_segment', 'steps', 'window')
SCALE_K = 7               # the property case: table(x 2^7) = table(x) 2^14


def shifts_table():
    """the DMAX shifts every handle takes a prefix of: bench_GMSK's bin table at DMAX bins"""
    conf = cfg.bench_config('bench_GMSK', blockSize=LOG2N, doppCarrierSteps=DMAX)
    _, _, shifts, _ = doppler_bin_table(conf['Radios']['Rx']['UHF-H'], conf['Radios']['rangeRateMax'], N)
    return np.asarray(shifts, dtype=np.int32)


def masks(bank):
    if bank == 'gmsk':
        conf = cfg.bench_config('bench_GMSK', blockSize=LOG2N, doppCarrierSteps=DMAX)
        _, m = loadProtocol('bench_GMSK')(conf=conf).get_filter(N, 16, 3)
        return np.asarray(m)
    rs = np.random.RandomState(SEEDS['t34'])
    h = np.zeros((8, N), dtype=np.complex128)
    h[:, :BANKS[bank]] = rs.standard_normal((8, BANKS[bank])) + 1j * rs.standard_normal((8, BANKS[bank]))
    return np.fft.fft(h, axis=1).astype(np.complex64)


def _unit(rs, n):
    return np.exp(2j * np.pi * rs.random_sample(n))


def inputs():
    """name -> complex64 block"""
    out = {'stream': sg.s1_stream(1, N, 1 << 10, 'GMSK', snr_db=8.0, seed=SEEDS['stream'])[:N]}
    # zero except one full-scale segment: the other segments of its slot have a largest component of 0 and the exponent 0
    x = np.zeros(N, dtype=np.complex128)
    x[SEG * V:SEG * V + 256] = _unit(np.random.RandomState(SEEDS['one_segment']), 256)
    out['one_segment'] = x
    # amplitude 2^0, 2^-1 ... 2^-20, 2^0 ... from segment to segment: the four segments of a slot carry four different scales
    k = (np.arange(N) // V) % 21
    out['steps'] = _unit(np.random.RandomState(SEEDS['steps']), N) * np.ldexp(1.0, -k)
    # a -60 dB floor and a full-scale burst on the last 47 and the first 48 samples of one segment: exactly its wrap window
    rs = np.random.RandomState(SEEDS['window'])
    x = 1e-3 * (rs.standard_normal(N) + 1j * rs.standard_normal(N)) / np.sqrt(2)
    x[SEG * V + 256 - 47:SEG * V + 256] = _unit(rs, 47)
    x[SEG * V:SEG * V + 48] = _unit(rs, 48)
    out['window'] = x
    return {k: np.asarray(v, dtype=np.complex64) for k, v in out.items()}


def main(bank_name, D, out):
    from pycusdr_amd.mfbank import MFBank
    m = masks(bank_name)
    bank = MFBank(LOG2N, D, m.shape[0])
    res = {}
    try:
        bank.set_filters(m)
        bank.set_shifts(shifts_table()[:D])
        info, path = bank.get_search_info(), bank.get_search_path()
        assert int(info['filter_side']) == 1 and path['log2L'] == 8 and path['valid_per_segment'] == V, (info, path)
        res['taps'], res['bins_per_forward'] = int(path['taps']), int(info['bins_per_forward'])
        for k, x in inputs().items():
            bank.upload(x)
            bank.find_carrier()
            res[f'scores_{k}'] = bank.get_scores()
        x = inputs()['stream']
        xk = (np.ldexp(x.real, SCALE_K) + 1j * np.ldexp(x.imag, SCALE_K)).astype(np.complex64)
        assert np.array_equal(np.ldexp(xk.real, -SCALE_K), x.real) and np.array_equal(np.ldexp(xk.imag, -SCALE_K), x.imag)
        bank.upload(xk)
        bank.find_carrier()
        res['scores_stream_scaled'] = bank.get_scores()
    finally:
        bank.close()
    np.savez(out, **res)


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3])
