"""numpy model of the wrap-around energy on the matrix cores (pycusdr_amd/csrc/wrap_kernels.hpp, k_segw).

The 256-point filter-side search subtracts, per (bin, segment), the energy of the L - V outputs whose filter support wraps
around the segment.  segf_body gets them from the product with the per-bin spectra and a pruned inverse transform; k_segw gets
them as a Toeplitz GEMM of the segment's edges with the per-bin shifted taps, in fp16 split into hi and lo halves with
power-of-two scales.  This model restates both, index for index, and checks that they agree.
"""
import numpy as np
import pytest

from seg_model import filter_support


def _bank(name, N=1 << 15):
    from pycusdr_amd import config as cfg
    from pycusdr_amd.protocol import loadProtocol
    ms = 5 if name == 'bench_BPSK' else 3
    conf = cfg.bench_config(name, blockSize=int(np.log2(N)), doppCarrierSteps=8)
    _, masks = loadProtocol(name)(conf=conf).get_filter(N, 16, ms)
    masks = np.asarray(masks)
    a, T, h = filter_support(masks)
    taps = h[:, (a + np.arange(T)) % N]
    # the unique rows (segf_body searches the unique filters; duplicates do not change the algebra)
    _, idx = np.unique(np.round(masks.view(np.float32), 6), axis=0, return_index=True)
    return taps[np.sort(idx)], N


def _geometry(T, L=256, NT=16):
    V = ((L - T + 1) // NT) * NT              # seg_valid: whole register slots
    Te = L - V + 1
    return V, Te


def wrap_via_transform(x_seg, taps_b, N, L, Te, V):
    """segf_body: v = N (x_seg (*) c') with c'[(r - (Te - 1)) mod L] = tap r; the energy of outputs [V, L) per filter (fp64)."""
    F, T = taps_b.shape
    cp = np.zeros((F, L), dtype=np.complex128)
    cp[:, (np.arange(T) - (Te - 1)) % L] = taps_b
    G = (N / L) * np.fft.fft(cp, axis=1)
    U = np.fft.fft(x_seg)
    v = np.fft.ifft(U[None, :] * G, axis=1) * L
    return (np.abs(v[:, V:]) ** 2).sum()


def toeplitz(x_seg, T, L, V, KT):
    """A[n'][r] = x_seg[(n' - r) mod L] for r < T, zero-padded to 16 KT taps (k_segw's window)."""
    n = np.arange(L - V)[:, None]
    r = np.arange(16 * KT)[None, :]
    A = x_seg[(n - r) % L]
    return np.where(r < T, A, 0)


def split16(v, e):
    """scale by 2^e, hi = fp16(v), lo = fp16(v - hi) (fp32 arithmetic, as on the device / host)."""
    s = np.ldexp(v.astype(np.float32), e).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def scale_exp(mx):
    """the power of two that brings the largest |component| into [2^14, 2^15)"""
    _, e = np.frexp(mx)
    return 15 - int(e)


def wrap_via_mfma_model(x_seg, taps_b, N, L, V, KT):
    """k_segw: the real-form GEMM [Xr Xi] [[Hr, Hi], [-Hi, Hr]] with the split-fp16 operands, fp32 accumulation of
    lo.hi + hi.lo + hi.hi (products exact in fp32), energy times 2^(2 log2 N - 2 e_a - 2 e_b)."""
    F, T = taps_b.shape
    A = toeplitz(x_seg, T, L, V, KT)
    # the window's samples actually read: offsets -(T - 1) ... L - V - 1
    win = x_seg[np.arange(-(T - 1), L - V) % L]
    ea = scale_exp(max(np.abs(win.real).max(), np.abs(win.imag).max()))
    Ar = np.concatenate([A.real, A.imag], axis=1)                     # (L - V) x 32 KT
    H = np.zeros((16 * KT, 8), dtype=np.complex128)
    H[:T, :F] = taps_b.T
    Br = np.block([[H.real, H.imag], [-H.imag, H.real]])             # 32 KT x 16: columns re of f, then im of f
    eb = scale_exp(max(np.abs(H.real).max(), np.abs(H.imag).max()))
    ah, al = split16(Ar, ea)
    bh, bl = split16(Br, eb)
    f32 = lambda m: m.astype(np.float32)
    C = (f32(al) @ f32(bh)).astype(np.float64) + (f32(ah) @ f32(bl)) + (f32(ah) @ f32(bh))
    lg = int(np.log2(N))
    return float((C ** 2).sum()) * 2.0 ** (2 * lg - 2 * ea - 2 * eb)


def _segments(L, rs):
    floor = 1e-3 * (rs.standard_normal(L) + 1j * rs.standard_normal(L))
    burst = floor.copy()
    burst[200:240] += 3.0 * np.exp(2j * np.pi * rs.random_sample(40))
    tone = np.exp(2j * np.pi * 0.0137 * np.arange(L))
    sparse = np.zeros(L, dtype=np.complex128)
    sparse[5] = 1.0 - 0.5j
    noise = rs.standard_normal(L) + 1j * rs.standard_normal(L)
    return [noise, burst, tone, sparse]


@pytest.mark.parametrize('name', ['bench_GMSK', 'bench_BPSK'])
def test_toeplitz_orientation_exact(name):
    """fp64: the Toeplitz form gives the transform's wrap energy (tap orientation, the Te - 1 offset, the window indices)."""
    taps, N = _bank(name)
    L = 256
    T = taps.shape[1]
    V, Te = _geometry(T)
    KT = -(-T // 16)
    rs = np.random.RandomState(1)
    for s in (0, 17, -301):
        hb = taps * np.exp(2j * np.pi * ((s * np.arange(T)) % N) / N)[None, :]
        for x_seg in _segments(L, rs):
            ref = wrap_via_transform(x_seg, hb, N, L, Te, V)
            C = toeplitz(x_seg, T, L, V, KT)[:, :T] @ hb.T
            got = N * N * (np.abs(C) ** 2).sum()
            assert abs(got - ref) <= 1e-10 * ref


@pytest.mark.parametrize('name', ['bench_GMSK', 'bench_BPSK'])
def test_split_fp16_gemm(name):
    """the split-fp16 GEMM gives the wrap energy within 5e-7 of the fp64 transform (GMSK 48 taps, BPSK 80 taps)."""
    taps, N = _bank(name)
    L = 256
    T = taps.shape[1]
    V, Te = _geometry(T)
    KT = -(-T // 16)
    rs = np.random.RandomState(2)
    worst = 0.0
    for s in (0, 5, 123, -77):
        hb = taps * np.exp(2j * np.pi * ((s * np.arange(T)) % N) / N)[None, :]
        for u in range(0, hb.shape[0], 8):
            hbu = hb[u:u + 8]
            for x_seg in _segments(L, rs):
                ref = wrap_via_transform(x_seg, hbu, N, L, Te, V)
                got = wrap_via_mfma_model(x_seg, hbu, N, L, V, KT)
                worst = max(worst, abs(got - ref) / ref)
    assert worst <= 5e-7, worst


def test_power_of_two_linearity():
    """score(4x) == 16 score(x) bit for bit: both scales are powers of two chosen from the data."""
    taps, N = _bank('bench_GMSK')
    T = taps.shape[1]
    V, _ = _geometry(T)
    x = np.random.RandomState(3).standard_normal(256) + 1j * np.random.RandomState(4).standard_normal(256)
    x = x.astype(np.complex64).astype(np.complex128)
    e1 = wrap_via_mfma_model(x, taps, N, 256, V, 3)
    e4 = wrap_via_mfma_model(4 * x, taps, N, 256, V, 3)
    assert e4 == 16 * e1


def test_geometry_at_the_edges_of_the_matrix_form():
    """13 valid register slots (V = 208) from 34 to 49 taps: 33 taps leave 14, and 49 taps are one more than three K-steps hold."""
    from seg_model import seg_valid, wrap_form
    assert [_geometry(T)[0] for T in (32, 33, 34, 48, 49, 50)] == [224, 224, 208, 208, 208, 192]
    assert all(seg_valid(T) == _geometry(T)[0] for T in range(1, 130))
    N, eight = 1 << 18, [1] * 8
    assert [wrap_form(N, eight, T, True) for T in (32, 33, 34, 48, 49, 50)] == ['vector', 'vector', 'matrix', 'matrix', 'vector', 'vector']
    assert wrap_form(N >> 1, eight, 48, True) == 'vector' and wrap_form(N << 2, eight, 48, True) == 'matrix'
    assert wrap_form(N, eight, 48, False) == 'vector' and wrap_form(N, [1] * 9, 48, True) == 'vector'
    assert wrap_form(N, [2, 1, 1], 48, True) == 'vector' and wrap_form(N, [2, 2, 2, 2], 48, True) == 'matrix'
    assert wrap_form(N, [2, 1, 1], 48, True, span_rank=3) == 'matrix' and wrap_form(N, [1] * 16, 48, True, span_rank=8) == 'matrix'
    assert wrap_form(N, [1] * 16, 48, True, span_rank=9) == 'vector' and wrap_form(N, eight, 48, True, log2L=11) == 'vector'


@pytest.mark.parametrize('T', [34, 40, 47, 48])
@pytest.mark.parametrize('rows', [1, 3, 6, 8])
def test_split_fp16_gemm_on_synthetic_banks(T, rows):
    """Where the device sweep goes (tests/tools/fuzz_wrap.py): complex normal taps of 34 ... 48 taps (three K-steps, the last one partly
    zero rows) in 1 ... 8 rows (unused tile columns), scaled over eight decades; noise segments, segments with one full-scale sample
    on a 1e-4 floor, segments scaled over thirty decades.  The wrap energy stays within the same 5e-7 of the fp64 transform."""
    N, L, KT = 1 << 18, 256, 3
    V, Te = _geometry(T)
    assert V == 208 and 16 * (KT - 1) < T <= 16 * KT
    rs = np.random.RandomState(1000 * T + rows)
    worst = {}
    for trial in range(3):
        taps = 10 ** rs.uniform(-6, 2) * (rs.standard_normal((rows, T)) + 1j * rs.standard_normal((rows, T)))
        s = int(rs.randint(0, N))
        hb = taps * np.exp(2j * np.pi * ((s * np.arange(T)) % N) / N)[None, :]
        noise = rs.standard_normal(L) + 1j * rs.standard_normal(L)
        spike = 1e-4 * (rs.standard_normal(L) + 1j * rs.standard_normal(L))
        spike[rs.randint(0, L)] = np.exp(2j * np.pi * rs.random_sample())
        edge = 1e-4 * (rs.standard_normal(L) + 1j * rs.standard_normal(L))
        edge[(rs.randint(-(T - 1), L - V)) % L] = np.exp(2j * np.pi * rs.random_sample())     # the full-scale sample inside the window
        scaled = 10 ** rs.uniform(-15, 15) * (rs.standard_normal(L) + 1j * rs.standard_normal(L))
        for kind, x_seg in (('noise', noise), ('spike', spike), ('spike', edge), ('scaled', scaled)):
            ref = wrap_via_transform(x_seg, hb, N, L, Te, V)
            got = wrap_via_mfma_model(x_seg, hb, N, L, V, KT)
            worst[kind] = max(worst.get(kind, 0.0), abs(got - ref) / ref)
    assert max(worst.values()) <= 5e-7, worst


def test_the_device_sweep_reaches_the_matrix_form():
    """tests/tools/fuzz_wrap.py's seeded draw, by the predicate alone: at least half of the cases take the matrix form, the four edge
    tap counts decide the form of the first four cases by themselves, and the corners the sweep is there for occur."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
    import fuzz_wrap as fw
    cs = fw.draw()
    assert len(cs) == fw.CASES >= 25
    assert [(c['T'], fw.expected(c, 'filters'), fw.expected(c, 'span')) for c in cs[:4]] == \
        [(33, 'vector', 'vector'), (34, 'matrix', 'matrix'), (48, 'matrix', 'matrix'), (49, 'vector', 'vector')]
    matrix = [c for c in cs if any(fw.expected(c, b) == 'matrix' for b in fw.bases(c))]
    assert 2 * len(matrix) >= len(cs)
    assert 2 * sum(fw.expected(c, 'filters') == 'matrix' for c in cs) >= len(matrix)
    assert {c['log2N'] for c in cs} == {18, 19, 20} and sum(c['log2N'] == 20 for c in cs) == 1
    assert sum(c['D'] >= 200 for c in cs) == 1 and all(1 <= c['D'] <= 40 for c in cs if c['D'] < 200)
    assert {c['M'] for c in cs} == {1, 2, 3, 5, 8, 16} and {c['dup'] for c in cs} == {'none', 'neg', 'twice'}
    assert {c['kind'] for c in cs} == {'noise', 'scaled', 'segment', 'spikes'} and {c['doff'] for c in matrix} == {0, 1}
    assert not all(c['sum_all'] for c in cs) and all(30 <= c['T'] <= 52 for c in cs)
    assert sum(c['start'] + c['T'] > (1 << c['log2N']) for c in matrix) >= 2            # taps that wrap around the end of the block
    # the default basis on the vector form and the span basis of the same handle on the matrix form: more than 8 unique filters, and
    # rows that do not count equally
    split = [c for c in cs if c['sum_all'] and (fw.expected(c, 'filters'), fw.expected(c, 'span')) == ('vector', 'matrix')]
    assert any(len(fw.counts(c)) > 8 for c in split) and any(c['dup'] == 'neg' for c in split)
    rows = {len(fw.counts(c)) for c in cs if fw.expected(c, 'filters') == 'matrix'} | {c['rank'] for c in cs if c['sum_all'] and fw.expected(c, 'span') == 'matrix'}
    assert {1, 2, 3, 5, 8} <= rows
