"""Child of tests/test_gpu_wrap_wide.py: tests/children/slots_child.py's `tables` at another block length -- 2^20 samples is the
smallest block at which the planner gives 256 bins the wide plan (four groups of 64 bins, 5040 one-slot waves).
usage: wide_child.py <log2N> <D> <out.npz>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slots_child                                                                     # noqa: E402

if __name__ == '__main__':
    slots_child.LOG2N = int(sys.argv[1])
    slots_child.N = 1 << slots_child.LOG2N
    out = {}
    slots_child.tables(int(sys.argv[2]), out)
    np.savez(sys.argv[3], **out)
