"""Writes tests/golden/segw_tables.npz, the fixture of tests/test_gpu_wrap_split.py: the doppSum tables of the matrix-core search
(k_segw) as the library scored them BEFORE the segment windows were split once per sample, and the fp64 oracle's tables of the same
blocks.  The tables in the committed file were written by commit fa0cd90 ("Channelise wideband IQ on the device"), the parent of the
change, on an MI355X; a later library must reproduce them bit for bit.

Inputs, banks and shifts are not stored: tests/children/split_child.py regenerates them from its seeds, which the file records
together with the parameters.  Stored per bank (gmsk: bench_GMSK, 48 taps; t34: 8 seeded filters of 34 taps):
  table_<bank>_<D>_<kind>   float32 [D]     column 0 of the device's table (the other columns are zero: a SUM_ALL search), D = 2 and 33
                                            on one-bin rectangles, D = 130 on forced 64,1 rectangles (chunks of 64, 64 and 2 bins)
  oracle_<bank>_<kind>      float64 [130]   column 0 of oracle.doppler_scores(fft(x), masks, shifts) -- the handles of D bins take the
                                            first D shifts

usage: python tests/golden/make_golden_segw.py oracle            (no GPU: about three minutes of transforms)
       python tests/golden/make_golden_segw.py device <commit>   (GPU, with the library of <commit>)
Each step rewrites its own arrays and keeps the other's; a last argument ending in .npz is written instead of the fixture."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'children'))
import split_child as sc                                                               # noqa: E402

OUT = os.path.join(HERE, 'segw_tables.npz')
CASES = ((2, '1,1'), (33, '1,1'), (130, '64,1'))           # (bins of the handle, forced rectangle)
DROP = ('MFB_SEG_FSM', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP', 'MFB_SEG_WRAP_MFMA')


def child_tables(bank, D, rect, out):
    """one child: the handle of D bins under the forced rectangle"""
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    env.update(MFB_SEG_WRAP_MFMA='1', MFB_SEG_FSM_RECT=rect)
    subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'children', 'split_child.py'), bank, str(D), out], check=True, env=env,
                   timeout=300)
    return dict(np.load(out))


def oracle(res):
    from oracle import mfbank_oracle as orc
    shifts = sc.shifts_table()
    xs = sc.inputs()
    for bank in sc.BANKS:
        m = sc.masks(bank)
        for k in sc.KINDS:
            res[f'oracle_{bank}_{k}'] = orc.doppler_scores(np.fft.fft(xs[k].astype(np.complex128)), m, shifts, True)[:, 0]
            print(f'oracle_{bank}_{k}', flush=True)


def device(res, commit):
    res['tables_commit'] = np.array(commit)
    with tempfile.TemporaryDirectory() as d:
        for bank in sc.BANKS:
            for D, rect in CASES:
                r = child_tables(bank, D, rect, os.path.join(d, f'{bank}_{D}.npz'))
                assert int(r['taps']) == sc.BANKS[bank] and int(r['bins_per_forward']) == int(rect.split(',')[0]), (bank, D, r['taps'])
                for k in sc.KINDS:
                    s = r[f'scores_{k}']
                    assert s.dtype == np.float32 and s.shape[0] == D and not s[:, 1:].any()
                    res[f'table_{bank}_{D}_{k}'] = s[:, 0].copy()


if __name__ == '__main__':
    res = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    res.update(log2N=sc.LOG2N, V=sc.V, dmax=sc.DMAX, segment=sc.SEG, scale_k=sc.SCALE_K,
               seeds=np.array([f'{k}={v}' for k, v in sorted(sc.SEEDS.items())]), taps=np.array([f'{k}={v}' for k, v in sorted(sc.BANKS.items())]))
    if sys.argv[1] == 'oracle':
        oracle(res)
    else:
        device(res, sys.argv[2])
    np.savez_compressed(sys.argv[-1] if sys.argv[-1].endswith('.npz') else OUT, **res)
