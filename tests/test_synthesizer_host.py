"""The synthesiser without a device (pycusdr_amd/synthesizer.py): the float64 model in its two forms, the host back end under cuts,
the refusals, the plan arithmetic of csrc/channelize_plan.hpp against its Python restatement, and the round trip of the model
through ``UniformChannelizer.model``."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import synth_scenes as sc
from pycusdr_amd import synthesizer as sy
from pycusdr_amd.channelizer import UniformChannelizer
from pycusdr_amd.synthesizer import UniformSynthesizer, check_plan_synthesis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'synthesize_plan_print.cpp')
FORM_SHAPES = [(8, 3, 37), (8, 8, 1), (16, 5, 17), (8, 2, 8)]


def scene(M, I, T, out_base, nout, seed=0):
    rs = np.random.RandomState(seed + M + T)
    h = (rs.uniform(-1, 1, T) / np.sqrt(T)).astype(np.float32)
    s = UniformSynthesizer(sc.FS, M, I, h, backend='host')
    first, count = s.needed_frames(out_base, nout)
    pl, need = sc.two_per_bin(s, sc.spread(M), first, count)
    s.set_source(sc.noise(rs, need))
    return s, pl


@pytest.mark.parametrize('M, I, T', FORM_SHAPES)
@pytest.mark.parametrize('out_base', [0, (1 << 40) + 3])
def test_the_two_forms_of_the_model_agree(M, I, T, out_base):
    nout = 40 * I + 5
    s, pl = scene(M, I, T, out_base, nout)
    direct, S = s.model(out_base, nout, pl)
    frames, S2 = s.model(out_base, nout, pl, form='frames')
    assert direct.shape == frames.shape == S.shape == (nout,) and np.array_equal(S, S2)
    has_taps = (out_base + np.arange(nout)) % I < T
    assert S[has_taps].min() > 0 and not S[~has_taps].any() and not direct[~has_taps].any()
    print(f'M {M} I {I} T {T}: the forms differ by {np.abs(direct - frames).max():.2e}')
    assert np.abs(direct - frames).max() <= 1e-12
    assert np.abs(direct).max() > 0.05


def test_the_model_is_the_zero_stuffed_filter_mixed_up():
    """the definition spelt out with np.convolve at out_base 0, one stream on bin 3 of 8"""
    M, I, T, b = 8, 3, 37, 3
    rs = np.random.RandomState(1)
    h = rs.uniform(-1, 1, T).astype(np.float32)
    s = UniformSynthesizer(sc.FS, M, I, h, backend='host')
    x = sc.noise(rs, 50)
    s.set_source(x)
    g = np.float32(0.37)
    w, _ = s.model(0, 190, [s.placement(b, 4, 0, 50, 0.37)])
    stuffed = np.zeros(54 * I, dtype=np.complex128)
    stuffed[4 * I::I] = (x.real * g) + 1j * (x.imag * g)
    ref = np.convolve(stuffed, h.astype(np.float64))[:190] * np.exp(2j * np.pi * b * np.arange(190) / M)
    assert np.abs(w - ref).max() <= 1e-13


@pytest.mark.parametrize('M, I, T', [(16, 5, 17), (8, 8, 1), (32, 7, 33)])
def test_host_back_end_is_bit_equal_under_uneven_cuts(M, I, T):
    base = 1001
    counts = (1, 2, I - 1, I, I + 1, 7 * I + 3, 40, 3)
    nout = sum(counts)
    s, pl = scene(M, I, T, base, nout, seed=3)
    whole = s.process(base, nout, pl)
    assert whole.dtype == np.complex64 and whole.shape == (nout,)
    assert np.array_equal(sc.bits(whole), sc.bits(s.model(base, nout, pl)[0].astype(np.complex64)))
    at = base
    for n in counts:
        assert np.array_equal(sc.bits(s.process(at, n, pl)), sc.bits(whole[at - base:at - base + n])), (at, n)
        at += n


def test_every_refusal_raises():
    h = np.ones(9, np.float32)
    for M in (4, 24, 512, 0):
        with pytest.raises(ValueError):
            check_plan_synthesis(M, 2, h)
    for I in (1, 0, 17):
        with pytest.raises(ValueError):
            check_plan_synthesis(16, I, h)
    for bad in (np.ones(0, np.float32), np.ones(4097, np.float32), np.r_[h, np.nan], np.r_[h, np.inf]):
        with pytest.raises(ValueError):
            check_plan_synthesis(16, 4, bad)
    with pytest.raises(ValueError):                      # 2048 frames of 9 complex64 do not fit
        check_plan_synthesis(8, 2, np.ones(4096, np.float32))
    assert check_plan_synthesis(16, 16, h)[:2] == (16, 16)
    with pytest.raises(ValueError):
        UniformSynthesizer(sc.FS, 16, 4, h, backend='eager')
    with pytest.raises(ValueError):
        UniformSynthesizer(sc.FS, 16, 4, h, backend='host', max_out=(1 << 24) + 1)
    with pytest.raises(ValueError):
        UniformSynthesizer(sc.FS, 16, 4, h, backend='host', max_frames=4097)
    s = UniformSynthesizer(sc.FS, 16, 4, h, backend='host', max_out=1000, max_frames=4)
    with pytest.raises(ValueError):
        s.process(0, 10, [])                             # no source
    with pytest.raises(ValueError):
        s.set_source(np.zeros(0, np.complex64))
    s.set_source(np.ones(100, np.complex64))
    for b in (-9, 16):
        with pytest.raises(ValueError):
            s.placement(b, 0, 0, 10)
    assert s.placement(-8, 0, 0, 10).bin == 8 and s.placement(15, 0, 0, 10).bin == 15
    P = s.placement
    for bad in ([P(1, -1, 0, 10)], [P(1, 0, -1, 10)], [P(1, 0, 0, 0)], [P(1, 0, 91, 10)], [P(1, 0, 0, 10, np.inf)], [P(1, 0, 0, 10, np.nan)],
                [P(1, 1 << 62, 0, 10)], [P(1, 0, 0, 10), P(1, 9, 10, 10)], [P(1, 20, 0, 10), P(2, 0, 0, 5), P(1, 11, 10, 10)],
                [P(1, 0, 0, 1)] * 5):
        with pytest.raises(ValueError):
            s.process(0, 10, bad)
        with pytest.raises(ValueError):
            s.model(0, 10, bad)
    for kw in (dict(out_base=-1), dict(out_count=0), dict(out_count=1001), dict(out_base=1 << 62)):
        with pytest.raises(ValueError):
            s.process(**dict(dict(out_base=0, out_count=10, placements=[]), **kw))
    # abutting, and the same span on two bins, are fine
    assert s.process(0, 10, [P(1, 0, 0, 10), P(1, 10, 10, 10), P(2, 0, 0, 10)]).shape == (10,)
    assert np.array_equal(s.freqs_hz, UniformChannelizer(sc.FS, 16, 4, h, backend='host').freqs_hz)


def test_every_plan_of_seventeen_frames_is_accepted_and_the_header_agrees_with_python(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    plans = []
    for M in sy.BINS:
        for I in sorted({2, 3, M // 2, M}):
            for J in (1, 2, 16, 17):
                for T in {min(4096, (J - 1) * I + 1), min(4096, J * I)}:
                    if -(-T // I) <= 17:
                        plans.append((M, I, T, True))
            for T in (18 * I, 40 * I, 300 * I, 4096):                 # beyond the promise: accepted or not, the two must agree
                if T <= 4096:
                    plans.append((M, I, T, False))
    assert {(256, 256, 4096), (256, 2, 34), (8, 2, 34), (256, 128, 2176)} <= {p[:3] for p in plans}
    exe = tmp_path / 'synthesize_plan_print'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', SRC, '-o', str(exe)], capture_output=True, text=True,
                           timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    calls = [(0, 1), (0, 1000), (7, 1000), ((1 << 40) + 3, 4097)]
    args = [f'{M}:{I}:{T}:{b}:{n}' for M, I, T, _ in plans for b, n in calls]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    got = [{k: int(v) for k, v in (kv.split('=') for kv in line.split())} for line in run.stdout.strip().splitlines()]
    assert len(got) == len(args)
    refused = 0
    for i, (M, I, T, promised) in enumerate(plans):
        F = sy.frames_per_workgroup(M, I, T)
        J = -(-T // I)
        for (b, n), g in zip(calls, got[len(calls) * i:]):
            assert (g['M'], g['I'], g['T'], g['kind'], g['D'], g['Tb'], g['threads']) == (M, I, T, 4, 1, J, 256)
            assert g['tile'] == g['F'] == F, (M, I, T)
            if F:
                assert g['rows'] == F + J - 1 and g['lds_bytes'] == sy.lds_bytes(M, I, T, F) <= 64 * 1024
                assert F == 128 or sy.lds_bytes(M, I, T, F + 1) > 64 * 1024
                assert g['grid'] == ((b + n - 1) // I - b // I) // F + 1
        if promised:
            assert F >= 1, (M, I, T)
            check_plan_synthesis(M, I, np.ones(T, np.float32))
        elif not F:
            refused += 1
            with pytest.raises(ValueError):
                check_plan_synthesis(M, I, np.ones(T, np.float32))
    assert refused > 0


def test_round_trip_of_the_two_models():
    """Synthesise three streams onto bins 2, 6 and 4 of 8 with I = 4, take them apart again with D = 4: each comes back 16 frames
    late within 1e-3 of the largest sample (1.2e-4 measured: the prototype's pass-band ripple and its stop band at the images)."""
    h, g, x = sc.round_trip_scene()
    assert len(h) == 65 and abs(float(g.sum()) - sc.RT_I) < 1e-5
    s = UniformSynthesizer(sc.FS, sc.RT_M, sc.RT_I, g, backend='host', max_source=x.size)
    s.set_source(x.reshape(-1))
    pl = [s.placement(b, 0, k * sc.RT_FRAMES, sc.RT_FRAMES) for k, b in enumerate(sc.RT_BINS)]
    nframes = sc.RT_FRAMES + sc.RT_DELAY
    w, _ = s.model(0, nframes * sc.RT_I, pl)
    uz = UniformChannelizer(sc.FS, sc.RT_M, sc.RT_I, h, bins=list(sc.RT_BINS), backend='host')
    y, _ = uz.model(0, w, 0, nframes)
    worst = np.abs(y[:, sc.RT_DELAY:] - x).max() / np.abs(x).max()
    print(f'round trip: worst deviation {worst:.2e} of the largest sample')
    assert worst <= 1e-3
    assert np.abs(y[:, :sc.RT_DELAY - 8]).max() <= 1e-3           # nothing arrives early
