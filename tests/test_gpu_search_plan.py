"""The plan of the segment search (pycusdr_amd/csrc/search_plan.hpp) on the device, on the smallest handle that reaches each form of
the main launch: what mfb_debug_search_plan reports for the handle is what the host-only planner gives for the inputs it reports,
mfb_get_search_info is a view of the same plan, and the search that plan launches scores a seeded block as the oracle does."""
import numpy as np
import pytest

from oracle import mfbank_oracle as orc
from pycusdr_amd import config as cfg, signals as sg
from pycusdr_amd.demodulator.demodulator_base import doppler_bin_table
from pycusdr_amd.mfbank import MFBank, debug_search_plan
from pycusdr_amd.protocol import loadProtocol

pytestmark = pytest.mark.gpu

SEG, SEGF256, SEGF2048, SEGW = 1, 2, 3, 4
# (protocol, log2N, bins, forced log2L or None, form of the main launch, log2L)
HANDLES = [('bench_GMSK', 15, 64, None, SEGF256, 8),      # rectangles shrunk to keep the chip full
           ('bench_GMSK', 18, 256, None, SEGW, 8),        # the smallest block on the matrix cores
           ('bench_BPSK', 15, 64, None, SEGF256, 8),      # 16 rows: no matrix-core form
           ('CC11xx', 15, 64, None, SEGF2048, 11),
           ('bench_GMSK', 15, 64, 9, SEG, 9)]             # time-side


def _oracle(X, masks, shifts):
    """orc.doppler_scores with the bins dealt to eight threads (numpy's transforms release the GIL; the rows are those of one call,
    bit for bit): the largest handle is 2048 fp64 inverse transforms of 2^18 points"""
    from concurrent.futures import ThreadPoolExecutor
    shifts = np.asarray(shifts)
    with ThreadPoolExecutor(8) as ex:
        return np.concatenate(list(ex.map(lambda c: orc.doppler_scores(X, masks, shifts[c], True), np.array_split(np.arange(len(shifts)), 8))))


@pytest.mark.parametrize('name,log2N,D,log2L,form,segl', HANDLES)
def test_the_handles_plan_is_the_planners_and_its_search_matches_the_oracle(name, log2N, D, log2L, form, segl):
    N = 1 << log2N
    conf = cfg.cc11xx_config(blockSize=log2N, doppCarrierSteps=D) if name == 'CC11xx' else cfg.bench_config(name, blockSize=log2N, doppCarrierSteps=D)
    sps, ms = (128, 3) if name == 'CC11xx' else (16, 5 if name == 'bench_BPSK' else 3)
    _, _, shifts, _ = doppler_bin_table(conf['Radios']['Rx']['UHF-H'], conf['Radios']['rangeRateMax'], N)
    M, masks = loadProtocol(name)(conf=conf).get_filter(N, sps, ms)
    x = sg.s1_stream(1, N, 1 << 10, 'GMSK', snr_db=8.0, seed=41)[:N].astype(np.complex64)
    bank = MFBank(log2N, D, M)
    try:
        bank.set_filters(masks)
        bank.set_shifts(shifts)
        if log2L:
            bank.set_search_path('segment', log2L=log2L)
        for nb in (1, 3):
            inputs, plan = bank.debug_search_plan(nb)
            assert debug_search_plan(inputs, nb) == (inputs, plan), nb          # the host-only planner, asked the same
            assert (plan['form'], plan['segl']) == (form, segl), plan
        inputs, plan = bank.debug_search_plan(1)
        info = bank.get_search_info()
        assert info == {'filter_side': form != SEG, 'bins_per_forward': plan['fb'] if form != SEG else 1}, (info, plan)
        if (name, log2N) == ('bench_GMSK', 15):
            assert inputs['T'] == 48 and (plan['fb'] < 16 if form == SEGF256 else plan['main_seg.grid'] > 0)
        bank.upload(x)
        bank.find_carrier()
        ds, X = bank.get_scores(), bank.get_spectrum()
    finally:
        bank.close()
    ref = _oracle(X, masks, shifts)
    err = np.abs(ds - ref).max() / ref.max()
    print(f'{name} 2^{log2N} x {D}: form {form}, {plan["fb"]} x {plan["fs"]} a wave, grid {plan["grid"] or plan["main_seg.grid"]}, score error {err:.2e}')
    assert err < 1e-5
