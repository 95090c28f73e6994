"""Child of tests/test_gpu_stream_edges.py: the byte forms of the stream search (k_stream_sync / k_stream_ring / k_stream_edges) on
the cases ``stream_cases.BYTE_CASES``.  The library reads MFB_STREAM_UNPACKED once per process, so they run in this process of their
own; it writes every batch's records to an .npz ('<case>|<batch>|<field>'), which the parent holds to the model and to the packed
kernel's records.
usage: stream_child.py <out.npz>"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import stream_cases as sc                                                             # noqa: E402
from pycusdr_amd.mfbank import MFBank                                                 # noqa: E402


def main(out):
    if not os.environ.get('MFB_STREAM_UNPACKED'):
        raise SystemExit('MFB_STREAM_UNPACKED is not set: this process would run the packed kernel')
    bank = MFBank(13, 4, 2)
    res = {}
    for name in sc.BYTE_CASES:
        assert sc.case(name).log2N == 13
        for i, rec in enumerate(sc.drive(sc.case(name), bank)[1]):
            res.update({f'{name}|{i}|{k}': v for k, v in rec.items()})
    np.savez(out, **res)
    bank.close()


if __name__ == '__main__':
    main(sys.argv[1])
