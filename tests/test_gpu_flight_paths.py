"""A flight -- one block (mfb_receive_block_begin) or a batch (mfb_receive_blocks_begin) -- takes one of six routes to the device:
plain launches, a graph just captured, a graph replayed, each on one stream or as two parts on two (mfb_set_batch_overlap).  Both
entries go through one launch function, and every route must hand back the same bytes: the same input is submitted again and
again with the same parameters (tests/children/flight_child.py; 2^15-sample blocks, 32 bins, bench_GMSK), one process -- with a
time limit of its own -- per (entry, overlap)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pycusdr_amd import _lib

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'flight_child.py')
LAY_FIELDS = [k for k, _ in _lib.RecordLayout._fields_]


def _run(tmp_path, kind):
    res = {}
    for overlap in (0, 1):
        out = str(tmp_path / f'{kind}{overlap}.npz')
        env = dict(os.environ)
        for k in ('MFB_NO_GRAPH', 'MFB_BATCH_SPLIT'):       # the switches that would take the routes away
            env.pop(k, None)
        subprocess.run([sys.executable, CHILD, kind, str(overlap), out], check=True, env=env, timeout=120)
        res[overlap] = dict(np.load(out))
    return res[0], res[1]


def _differing(a, b):
    return int(np.count_nonzero(np.asarray(a).view(np.uint8) != np.asarray(b).view(np.uint8)))


@pytest.mark.gpu
def test_single_block_is_the_same_on_every_route(tmp_path):
    """mfb_block_result and the three arrays (and the two SNR windows) of calls 1 (plain launches), 2 (captured and launched), 3 and 4
    (replayed), on one stream and on two: all equal, byte for byte."""
    one, two = _run(tmp_path, 'block')
    n, (l0, l1) = int(one['count']), (int(v) for v in one['band_len'])
    print(f'count {n}, band_len {l0} {l1}')
    assert n > 1900 and l0 > 0 and l1 > 0          # a block inside the packet: there is something to compare
    ref = {k: one[k][0] for k in ('result', 'sym', 'cen', 'mag', 'bands')}
    for name, r in (('one stream', one), ('two streams', two)):
        for call in range(4):
            for k, v in ref.items():
                d = _differing(r[k][call], v)
                print(f'{name}, call {call + 1}, {k}: {d} bytes differ from call 1 on one stream')
                assert d == 0, (name, call, k)


@pytest.mark.gpu
def test_batch_records_are_the_same_on_every_route(tmp_path):
    """The raw record bytes and the mfb_record_layout of mfb_receive_blocks_end_record, stream stages on, the carry seeded afresh
    before every call: equal across plain launches, capture and replay (four calls per carry parity -- the graphs are kept per
    parity), on one stream and on two.  The layout equals, field for field, what mfb_debug_stream_stages reports on the same handle
    for the same symbol count (band capacity 0, the same number of blocks: every field is comparable)."""
    one, two = _run(tmp_path, 'batch')
    lay = dict(zip(LAY_FIELDS, one['layouts'][0].tolist()))
    print(lay)
    assert lay['nblocks'] == 3 and lay['stream_stages'] == 1 and lay['band_capacity'] == 0 and lay['templates'] == 2
    assert one['records'].shape == (8, 3 * lay['record_bytes'])
    rec0 = one['records'][0].reshape(3, lay['record_bytes'])
    bits = rec0[:, lay['off_bits']:lay['off_bits'] + lay['symbols']]
    assert bits.any() and rec0[:, lay['off_sym']:lay['off_sym'] + 4 * lay['symbols']].any()      # the stages and the centres ran
    for name, r in (('one stream', one), ('two streams', two)):
        for call in range(8):
            d = _differing(r['records'][call], one['records'][0])
            print(f'{name}, call {call + 1}: {d} record bytes differ from call 1 on one stream')
            assert d == 0, (name, call)
            assert r['layouts'][call].tolist() == one['layouts'][0].tolist(), (name, call)
        assert dict(zip(LAY_FIELDS, r['debug_layout'].tolist())) == lay, name
