"""tests/stream_model.py (the reference the stream-stage kernels are held to in tests/test_gpu_stream_edges.py) against what it
restates -- the reference's recorded KATs (fixtures G7) and ``demodulateHost`` of a real Demodulator at the geometry of
tests/test_gpu_stream_stages.py -- and the case table of tests/stream_cases.py through the model alone: every case reaches the branch
it is named for.  No GPU."""
import numpy as np
import pytest

from pycusdr_amd import config as cfg
from pycusdr_amd.demodulator import UHF
from pycusdr_amd.protocol import loadProtocol
import pycusdr_amd.demodulator.demodulator_base as dbm

import stream_cases as sc
from oracle_bank import OracleBank
from stream_model import StreamModel, STATUS
from test_gpu_stream_stages import _blocks, _host_block, BS, OV, N


def _mag_of(trust, n):
    """float32 magnitudes whose leading bytes are `trust` (quirk Q3)"""
    raw = np.zeros(4 * n, dtype=np.int8)
    raw[:len(trust)] = trust
    return raw.view(np.float32)


@pytest.mark.parametrize('scenario', ['aligned', 'early', 'late', 'both', 'short'])
def test_model_reproduces_the_overlap_kats(goldens, scenario):
    ov = int(goldens[f'g7/overlap/{scenario}/ov'])
    m = StreamModel(1 << 12, ov, 20, 10, 1000, np.array([0, 1], np.uint8))
    m.seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    seen = []
    for b in range(4):
        k = f'g7/overlap/{scenario}/b{b}'
        bits = goldens[f'{k}/bits']
        r = m.batch([(len(bits), bits.astype(np.int32), goldens[f'{k}/centres'].astype(np.int32), _mag_of(goldens[f'{k}/trust'], len(bits)))])[0]
        assert r['host_error'] is None
        assert np.array_equal(r['bits'], goldens[f'{k}/bitsWin'].astype(np.uint8))
        assert np.array_equal(r['cen8'], goldens[f'{k}/centresWin'].astype(np.uint8))
        assert np.array_equal(r['trust'], goldens[f'{k}/trustWin'].astype(np.uint8))
        seen.append(r['tag'])
    if scenario in ('early', 'late', 'both'):
        assert any(t.startswith('repaired') for t in seen), seen
    if scenario == 'aligned':
        assert set(seen) == {'device-expected'}, seen


def test_model_reproduces_the_nrzs_kat(goldens):
    lut = np.asarray(loadProtocol('bench_BPSK')(conf=cfg.bench_config('bench_BPSK')).get_symbolLUT2(5)[1])
    sym = goldens['g7/nrzs/symbols'].astype(np.int32)
    n = len(sym)
    cen = np.linspace(100, 3997, n).astype(np.int32)          # everything but the last symbol inside the window
    m = StreamModel(1 << 12, 200, 20, 10, 10 ** 6, lut)
    m.seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    r = m.batch([(n, sym, cen, np.zeros(n, np.float32))])[0]
    assert r['tag'] == 'device-expected' and r['start'] == 0 and r['nwin'] == n - 1
    assert np.array_equal(r['bits'], goldens['g7/nrzs/bits'].astype(np.uint8)) and r['noerr'] == len(goldens['g7/nrzs/symError'])


@pytest.mark.parametrize('mode,pname', [('lut', 'bench_GMSK'), ('nrzs', 'bench_BPSK')])
def test_model_equals_demodulate_host_at_the_seam_tests_geometry(monkeypatch, mode, pname):
    """2^15 samples, overlap 2^10, 16 samples per symbol, the protocols' own constants: the same arrays and the same state as
    ``demodulateHost`` of a real Demodulator, block by block, planted slips and every kind of irregular block included."""
    monkeypatch.setattr(dbm, 'MFBank', OracleBank)
    conf = cfg.bench_config(pname, blockSize=BS, doppCarrierSteps=8)
    host = UHF.Demodulator(conf, loadProtocol(pname)(conf=conf), 'UHF-H')
    lut = host._bitLUT_u8 if mode == 'lut' else host.symbolLUT
    m = StreamModel(N, host.sigOverlap, host.overlapOffset, host.symbol_check_match_threshold, host.symbol_check_error_threshold, lut)
    assert host.sigOverlap == OV
    m.seed(np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    slips = {3: 1, 7: -1, 8: -1, 14: 1, 15: 1}
    irregular = {5: 'negative', 10: 'large', 12: 'no_end', 16: 'tiny', 18: 'no_start'}
    blocks = _blocks(np.random.RandomState(12), mode, 20, lut, slips, irregular)
    seen = []
    for b, blk in enumerate(blocks):
        got, err = _host_block(host, blk)
        r = m.batch([blk])[0]
        seen.append(r['tag'])
        assert (err is None) == (r['host_error'] is None), (b, err, r['host_error'])
        if b in irregular:
            assert r['tag'] == 'irregular', (b, r['tag'])
        if err is None:
            assert all(np.array_equal(r[k], g) for k, g in zip(('bits', 'cen8', 'trust'), got)), b
            assert np.array_equal(r['post'], np.asarray(host.poswinP).astype(np.uint8)), b
            assert np.array_equal(r['end'], np.asarray(host.posSymEnd).astype(np.uint8)), b
        m.seed(*m.host_state()[:2])              # (as the seam test seeds every batch from the host's state)
    assert 'repaired +1' in seen and 'repaired -1' in seen, seen
    host.close()


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_every_case_reaches_the_branch_it_is_named_for(name):
    c = sc.case(name)
    batches = sc.model_results(name)
    assert len(batches) == sum(s[0] == 'batch' for s in c.steps)
    for res in batches:
        for r in res:
            assert r['status'] == STATUS[r['tag']]
            # a caught exception of the alignment is the raise path; the one exception: a previous tail of ONE bit, which numpy
            # broadcasts -- it raises later or (a block already aligned) not at all, and adjusts nothing either way
            if r['host_logged'] and r['tag'] != 'irregular':
                assert r['tag'] == 'raised', (name, r['tag'])
            if r['tag'] == 'raised' and not r['host_logged']:
                assert r['prev_npost'] == 1, (name, r['prev_npost'])
    c.reach(batches)


def test_case_table_covers_every_status_and_tag():
    seen = set()
    for name in sc.CASES:
        seen |= set(sc.tags(sc.model_results(name)))
    assert seen == set(STATUS), seen
