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
