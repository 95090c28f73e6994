"""The receive loop (DemodulatorRunner.run_stream, B blocks per device call, no decoder) on a recording of integer samples, three
ways: complex64 chunks (converted before the clock starts: the loop as it always was), int16 chunks taken natively
("sample_format": "sc16": converted on the device), and int16 chunks converted on the loop's thread with astype -- what a caller
with a real radio had to do before.  Medians of --reps runs (profiles/sample_format.md).
usage: python3 tools/sample_format_rate.py [log2N] [bins] [B] [blocks] [--reps R] [--chunk samples]"""
import copy
import sys
import time
import numpy as np
sys.path.insert(0, '.')
from pycusdr_amd.hostcpu import quiet_blas  # noqa: E402
quiet_blas()
from pycusdr_amd import config as cfg, signals as sg  # noqa: E402
from pycusdr_amd.demodulator_process import DemodulatorRunner  # noqa: E402
from pycusdr_amd.protocol import loadProtocol  # noqa: E402


def _option(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        value = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return value
    return default


reps = int(_option('--reps', 5))
chunk = int(_option('--chunk', 16384))
log2N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
D = int(sys.argv[2]) if len(sys.argv) > 2 else 64
B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
nblocks = int(sys.argv[4]) if len(sys.argv) > 4 else 40 * B
N, ov = 1 << log2N, 1 << 10
conf = cfg.bench_config('bench_GMSK', blockSize=log2N, doppCarrierSteps=D)
conf['GPU']['UHF'].setdefault('HIP', {})['blocks_per_call'] = B
confI = copy.deepcopy(conf)
confI['GPU']['UHF']['HIP'].update(sample_format='sc16', sample_scale=2.0 ** -11)
p = loadProtocol('bench_GMSK')(conf=conf)
sig = sg.s1_stream(nblocks, N, ov, 'GMSK', snr_db=12.0, seed=3)[ov:]
q = np.clip(np.round(np.stack((sig.real, sig.imag), axis=1) * 2.0 ** 11), -32768, 32767).astype(np.int16)
x = (q.astype(np.float32) * np.float32(2.0 ** -11)).view(np.complex64).reshape(len(q))
q.flags.writeable = x.flags.writeable = False       # a recording: its chunks may be copied by the copy thread
step = np.float32(2.0 ** -11)


def converted():
    for i in range(0, len(q), chunk):
        c = (q[i:i + chunk].astype(np.float32) * step).view(np.complex64).reshape(-1)
        c.flags.writeable = False
        yield c


cases = (('cf32 chunks', conf, lambda: (x[i:i + chunk] for i in range(0, len(x), chunk))),
         ('sc16 chunks, converted on the device', confI, lambda: (q[i:i + chunk] for i in range(0, len(q), chunk))),
         ('sc16 chunks, astype on the loop\'s thread', conf, converted))
for name, c, source in cases:
    run = DemodulatorRunner(c, p, 'UHF-H')
    run.run_stream(source())                       # graphs recorded, clock settled
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res, _ = run.run_stream(source())
        dt = time.perf_counter() - t0
        rates.append(len(res) * (N - ov) / dt / 1e6)
    print(f'N=2^{log2N} D={D} B={B} chunks of {chunk}: {name:42s} median of {reps}: {float(np.median(rates)):8.1f} Msamples/s '
          f'({min(rates):.1f} ... {max(rates):.1f})', flush=True)
    run.close()
