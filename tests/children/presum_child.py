"""Child of tests/test_gpu_presum_rows.py: one handle of 33 bins at 2^18 samples (bench_GMSK) whose partial sums are written by one
search form after another, a table taken after each step, and fresh handles to compare with.  Writes an .npz.
usage: presum_child.py steps <sum_all: 0|1> <out.npz>    default basis, span, filters, two-pass path, auto -- on ONE handle
       presum_child.py batch <out.npz>                   three blocks of a window as one batch, and the same blocks one per call"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wrap_child import cfg, doppler_bin_table, loadProtocol, sg, MFBank                # noqa: E402
from pycusdr_amd.demodulator import UHF, Operations                                    # noqa: E402

NAME, LOG2N, D = 'bench_GMSK', 18, 33
N = 1 << LOG2N


def _handle(sum_all, basis='filters', path='auto'):
    conf = cfg.bench_config(NAME, blockSize=LOG2N, doppCarrierSteps=D)
    _, _, shifts, _ = doppler_bin_table(conf['Radios']['Rx']['UHF-H'], conf['Radios']['rangeRateMax'], N)
    M, masks = loadProtocol(NAME)(conf=conf).get_filter(N, 16, 3)
    bank = MFBank(LOG2N, D, M, sum_all_masks=sum_all)
    bank.set_filters(masks)
    bank.set_shifts(shifts)
    if basis != 'filters':
        bank.set_search_basis(basis)
    if path != 'auto':
        bank.set_search_path(path)
    return bank


def _table(bank, x):
    bank.upload(x)
    bank.find_carrier()
    return bank.get_scores()


def steps(sum_all, res):
    x = sg.s1_stream(1, N, 1 << 10, 'GMSK', snr_db=8.0, seed=41)[:N].astype(np.complex64)
    live = _handle(sum_all)
    try:
        res['path_default'] = live.get_search_path()['path']
        res['filter_side'] = int(live.get_search_info()['filter_side'])
        res['live_default'] = _table(live, x)
        if sum_all:
            live.set_search_basis('span')
            res['span_rows'] = live.get_search_basis()[1]
            res['live_span'] = _table(live, x)
            live.set_search_basis('filters')
        else:
            try:
                live.set_search_basis('span')
                res['span_refused'] = 0
            except Exception:
                res['span_refused'] = 1
        res['live_filters'] = _table(live, x)
        live.set_search_path('twopass')
        res['path_twopass'] = live.get_search_path()['path']
        res['live_twopass'] = _table(live, x)
        live.set_search_path('auto')
        res['path_auto'] = live.get_search_path()['path']
        res['live_auto'] = _table(live, x)
    finally:
        live.close()
    for name, kw in (('default', {}), ('span', dict(basis='span')), ('twopass', dict(path='twopass'))):
        if name == 'span' and not sum_all:
            continue
        f = _handle(sum_all, **kw)
        try:
            res[f'fresh_{name}'] = _table(f, x)
        finally:
            f.close()


def batch(res):
    ov, nb = 1 << 10, 3
    step = N - ov
    conf = cfg.bench_config(NAME, blockSize=LOG2N, doppCarrierSteps=D)
    sig = sg.s1_stream(nb, N, ov, 'GMSK', snr_db=9.0, seed=23)[:nb * step + ov].astype(np.complex64)
    bat, one = (UHF.Demodulator(conf, loadProtocol(NAME)(conf=conf), 'UHF-H') for _ in range(2))
    K = dict(k_offset=bat.codeRateAndPhaseOffsetHigh, k_len=bat.codeRateAndPhaseOffsetLow - bat.codeRateAndPhaseOffsetHigh,
             spsym_min=bat.spsymMin, op=Operations.CENTRES_ABS.value)
    try:
        res['filter_side'] = int(bat.bank.get_search_info()['filter_side'])
        # the batch handle has searched one block on the span basis before: other sums in the rows the default form does not write
        bat.bank.set_search_basis('span')
        _table(bat.bank, sig[:N])
        bat.bank.set_search_basis('filters')
        bat.bank.windows(nb, step)[0][:] = sig
        bat.bank.begin_blocks(0, nb, **K)
        blocks = bat.bank.end_blocks(0)
        assert len(blocks) == nb
        for b in range(nb):
            res[f'batch_scores{b}'] = bat.bank.get_batch_scores(b)
            one.bank.input[:] = sig[b * step:b * step + N]
            one.bank.receive_block(**K)
            res[f'single_scores{b}'] = one.bank.get_scores()
    finally:
        bat.close()
        one.close()


if __name__ == '__main__':
    out = {}
    if sys.argv[1] == 'steps':
        steps(bool(int(sys.argv[2])), out)
    else:
        batch(out)
    np.savez(sys.argv[-1], **out)
