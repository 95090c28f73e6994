"""The soft combiner on the device (mfb_combiner_*, csrc/combine_kernels.hpp) against the host back end and the recordings of
the reference's own SoftCombiner (tests/golden/ref_goldens_combiner.npz)."""
import numpy as np
import pytest

import combiner_common as cc

pytestmark = pytest.mark.gpu

VM, MINLEN, WEIGHT = 15.0, 200, 1.2


def _combiner(max_bits=1 << 13, weight=WEIGHT):
    from pycusdr_amd import mfbank, softCombiner as sc
    c = mfbank.Combiner(max_bits=max_bits)
    for v in (2, 3, 4):
        c.set_vote(v, *sc.vote_table(v, weight))
    return c


def _aligned_case(rs, Lm, lens, offsets, flip=0.1):
    """A master of Lm random bits and slaves that hold it, 10 % of the bits flipped, at the given offsets of buffers of the
    given lengths; random trust of every class."""
    def trust(n):
        return rs.choice(np.array([-128, -5, -2, -1, -1, 0, 0, 1, 3, 127], dtype=np.int8), n)
    m = rs.randint(0, 2, Lm).astype(np.int8)
    slaves = []
    for n, off in zip(lens, offsets):
        b = rs.randint(0, 2, n).astype(np.int8)
        k = min(Lm, n - off)
        b[off:off + k] = m[:k] ^ (rs.random_sample(k) < flip)
        slaves.append((b, trust(n)))
    return m, trust(Lm), slaves


def test_bit_xcorr_equals_the_exact_integer_correlation():
    """mfb_debug_bit_xcorr == np.rint of the float64 FFT form at all N lags: buffer lengths below, at and above a power of
    two, master lengths around the 32-bit word, one bit, and longer than the buffer (only its first n bits count)."""
    from pycusdr_amd import mfbank
    rs = np.random.RandomState(11)
    for n in (1000, 1024, 1025, 4097, 58834):
        a = rs.randint(0, 2, n).astype(np.uint8)
        N = 1 << int(np.ceil(np.log2(n)))
        A = np.fft.fft(np.r_[a, np.zeros(N - n)].astype(np.float64))
        for m in (1, 31, 32, 33, 999, n + 77):
            b = rs.randint(0, 2, m).astype(np.uint8)
            if m == 1:
                b[:] = 1
            want = np.rint(np.fft.ifft(A * np.conj(np.fft.fft(b[:n].astype(np.float64), N))).real).astype(np.int64)
            got = mfbank.bit_xcorr(a, b)
            assert got.dtype == np.int32 and got.shape == (N,)
            assert np.array_equal(got, want), (n, m, int(np.abs(got - want).max()))


@pytest.mark.parametrize('name', cc.SCENARIOS)
def test_scenario_hip_equals_host_and_the_reference(name):
    """Every recorded scenario on the hip back end: the reference's result and indices byte for byte, and the core's record
    equal to the host's -- val[15], idx0, avail and cond, the float64 bit for bit -- without the host path being taken."""
    from pycusdr_amd import softCombiner as sc
    res, ws, comb = cc.run_scenario(name, 'hip')
    cc.check_against_reference(name, res, ws)
    args = cc.core_inputs(name)
    cc.same_core(comb.combine(*args), sc.combine_host(*args, VM, WEIGHT, MINLEN), cond_rel=0.0)
    assert comb.host_fallbacks == 0
    comb.close()


def test_randomised_vote_against_the_tables():
    """10 000 columns for 2, 3 and 4 voters, three weights: the device's vote is the table entry of every column's state."""
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(5)
    L = 10000
    for w in cc.WEIGHTS:
        c = _combiner(1 << 14, w)
        for K in (1, 2, 3):
            offs = [17, 1000, 333][:K]
            m, t, slaves = _aligned_case(rs, L, [L + 1500] * K, offs)
            res = c.combine(m, t, slaves, VM, MINLEN)
            assert res['status'] == sc.COMBINED and res['matched'] == list(range(K)) and len(res['bits']) == L
            assert [r['idx0'] for r in res['slaves']] == offs
            s = sc.column_states([m] + [b[o:o + L] for (b, _), o in zip(slaves, offs)], [t] + [tt[o:o + L] for (_, tt), o in zip(slaves, offs)])
            tb, tt = sc.vote_table(K + 1, w)
            assert np.array_equal(res['bits'], tb[s]) and np.array_equal(res['trust'], tt[s]), (w, K)
        c.close()


def test_begin_end_overlap_with_a_second_handle():
    from pycusdr_amd import softCombiner as sc
    a, b = _combiner(), _combiner()
    ia, ib = cc.core_inputs('a_two_slaves'), cc.core_inputs('c_second_slave_ends_early')
    a.begin(*ia, VM, MINLEN)
    b.begin(*ib, VM, MINLEN)
    rb = b.end()
    ra = a.end()
    cc.same_core(ra, sc.combine_host(*ia, VM, WEIGHT, MINLEN), cond_rel=0.0)
    cc.same_core(rb, sc.combine_host(*ib, VM, WEIGHT, MINLEN), cond_rel=0.0)
    a.close()
    b.close()


def test_misuse_returns_the_documented_errors():
    import ctypes as C
    from pycusdr_amd import _lib, mfbank
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mfb_combiner_create(C.byref(h), 0, 0, 3) == _lib.MFB_ERR_ARG
    assert lib.mfb_combiner_create(C.byref(h), 0, 1024, -1) == _lib.MFB_ERR_ARG
    assert lib.mfb_combiner_create(C.byref(h), 0, (1 << 20) + 1, 3) == _lib.MFB_ERR_UNSUPPORTED
    assert lib.mfb_combiner_create(C.byref(h), 0, 1024, 4) == _lib.MFB_ERR_UNSUPPORTED
    assert lib.mfb_combiner_create(None, 0, 1024, 3) == _lib.MFB_ERR_ARG
    assert not h
    assert lib.mfb_combiner_destroy(None) == _lib.MFB_ERR_ARG
    m, t, slaves = cc.core_inputs('a_two_slaves')
    c = mfbank.Combiner(max_bits=1 << 13, max_slaves=2)
    with pytest.raises(_lib.MFBankError):                  # end without begin
        c.end()
    with pytest.raises(_lib.MFBankError):                  # vote tables not set
        c.begin(m, t, slaves, VM, MINLEN)
    from pycusdr_amd import softCombiner as sc
    tb, tt = sc.vote_table(2, WEIGHT)
    with pytest.raises(ValueError):                        # 8^3 entries for 3 voters
        c.set_vote(3, tb, tt)
    with pytest.raises(ValueError):
        c.set_vote(5, tb, tt)
    for v in (2, 3, 4):
        c.set_vote(v, *sc.vote_table(v, WEIGHT))
    p = _lib.CombineParams(VM, MINLEN, 0, 0)
    mb, mt = m.view(np.uint8), t
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)        # noqa: E731
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), None, None) == _lib.MFB_ERR_ARG       # master length 0
    p.master_len = (1 << 13) + 1
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), None, None) == _lib.MFB_ERR_ARG       # beyond max_bits
    p.master_len, p.num_slaves = len(mb), 1
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), None, None) == _lib.MFB_ERR_ARG       # no slave arrays
    sb = (C.c_void_p * 3)(*[b.ctypes.data for b, _ in slaves], None)
    st = (C.c_void_p * 3)(*[x.ctypes.data for _, x in slaves], None)
    p.slave_len[0] = 0
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), sb, st) == _lib.MFB_ERR_ARG           # slave length 0
    p.num_slaves = 3
    p.slave_len[0] = p.slave_len[1] = p.slave_len[2] = 16
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), sb, st) == _lib.MFB_ERR_ARG           # more than max_slaves
    p.num_slaves = 4
    assert lib.mfb_combiner_begin(c._h, C.byref(p), ptr(mb), ptr(mt), sb, st) == _lib.MFB_ERR_UNSUPPORTED   # more than three
    assert lib.mfb_combiner_begin(c._h, None, ptr(mb), ptr(mt), sb, st) == _lib.MFB_ERR_ARG
    R = _lib.CombineResult()
    assert lib.mfb_combiner_end(c._h, C.byref(R), ptr(mb), ptr(mt)) == _lib.MFB_ERR_STATE                   # nothing was begun
    c.begin(m, t, slaves, VM, MINLEN)
    with pytest.raises(_lib.MFBankError):                  # one call in flight per combiner
        c.begin(m, t, slaves, VM, MINLEN)
    assert lib.mfb_combiner_set_vote(c._h, 2, ptr(tb), ptr(tt), 64) == _lib.MFB_ERR_STATE
    assert lib.mfb_combiner_end(c._h, None, None, None) == _lib.MFB_ERR_ARG
    assert c.end()['status'] == sc.COMBINED                # and the handle still works
    out = np.empty(1024, np.int32)
    assert lib.mfb_debug_bit_xcorr(0, ptr(mb), 0, ptr(mb), 5, ptr(out)) == _lib.MFB_ERR_ARG
    assert lib.mfb_debug_bit_xcorr(0, ptr(mb), 5, ptr(mb), (1 << 20) + 1, ptr(out)) == _lib.MFB_ERR_UNSUPPORTED
    c.close()


def test_four_slaves_take_the_host_path():
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(8)
    m, t, slaves = _aligned_case(rs, 1501, [3001, 2999, 3003, 2503], [100, 700, 31, 1000])
    hip = sc.SoftCombiner(cc.conf_of(), backend='hip')
    got = hip.combine(m, t, slaves)
    assert hip.host_fallbacks == 1 and hip._combiner is None
    assert got['matched'] == [0, 1, 2, 3] and got['status'] == sc.COMBINED
    cc.same_core(got, sc.combine_host(m, t, slaves, VM, WEIGHT, MINLEN))
    got3 = hip.combine(m, t, slaves[:3])                    # three slaves: the device again
    assert hip.host_fallbacks == 1 and hip._combiner is not None
    cc.same_core(got3, sc.combine_host(m, t, slaves[:3], VM, WEIGHT, MINLEN), cond_rel=0.0)
    hip.close()


def test_handle_reuse_equals_fresh_handles():
    """50 calls of changing shapes -- lengths across word and power-of-two borders, 0 to 3 slaves, matched, unrelated, cut
    short, too short to evaluate, growth beyond the handle's first size -- on one handle and on a fresh one each."""
    from pycusdr_amd import softCombiner as sc
    rs = np.random.RandomState(21)
    one = _combiner(1 << 11)
    statuses = set()
    for call in range(50):
        Lm = int(rs.choice([1000, 1023, 1024, 1025, 1500, 2047, 2049, 3000]))
        K = call % 4
        lens = [int(rs.choice([15, 1024, 1500, 2048, 2500, 4095, 4097])) for _ in range(K)]
        offs = [int(rs.randint(0, max(1, n - 150))) for n in lens]
        m, t, slaves = _aligned_case(rs, Lm, lens, offs, flip=0.05)
        if K and call % 7 == 0:
            slaves[0] = (rs.randint(0, 2, lens[0]).astype(np.int8), slaves[0][1])       # unrelated
        if K and call % 9 == 4:            # a 1024-bit buffer the master runs round the end of: matched at lag 900, 124 bits left
            b = np.roll(np.r_[m, rs.randint(0, 2, 24).astype(np.int8)][:1024], 900)
            slaves[-1] = (b, slaves[-1][1][:1].repeat(1024))
        got = one.combine(m, t, slaves, VM, MINLEN)
        fresh = _combiner(1 << 13)
        want = fresh.combine(m, t, slaves, VM, MINLEN)
        fresh.close()
        cc.same_core(got, want)
        if call % 10 == 0:
            cc.same_core(got, sc.combine_host(m, t, slaves, VM, WEIGHT, MINLEN), cond_rel=0.0)
        statuses.add(got['status'])
    assert statuses == {sc.NOTHING, sc.COMBINED, sc.MASTER_ONLY}
    one.close()


def test_three_channels_through_one_compare_workers_round():
    """The geometry of test_three_channels_in_three_threads_one_device (three modulations, 2^15-sample blocks, one device):
    every channel's result dicts go into a hip and a host SoftCombiner as one worker each; compareWorkers gives identical
    dicts on both back ends, round after round."""
    from pycusdr_amd import config as cfg, signals as sg, softCombiner as sc
    from pycusdr_amd.demodulator_process import DemodulatorRunner
    from pycusdr_amd.protocol import loadProtocol
    bs, ov = 15, 1 << 10
    N = 1 << bs
    per_channel = []
    for k, (mod, pname) in enumerate([('GMSK', 'bench_GMSK'), ('FSK', 'bench_FSK'), ('BPSK', 'bench_BPSK')]):
        sig = sg.awgn(np.concatenate((sg.get_padded_packet(mod)[0], np.zeros(2 * N))), 12.0, rng=np.random.RandomState(40 + k)).astype(np.complex64)
        conf = cfg.bench_config(pname, blockSize=bs, doppCarrierSteps=48)
        run = DemodulatorRunner(conf, loadProtocol(pname)(conf=conf), 'UHF-H')
        res, _ = run.run_stream((sig[i:i + 4096] for i in range(0, len(sig), 4096)))
        run.close()
        per_channel.append([{**r, 'workerId': f'rx-{mod}', 'voteGroup': 0} for r in res])
    assert all(len(c) >= 2 for c in per_channel)
    now = [0.0]
    conf = cc.conf_of(min_length=1000, threshold=3)
    conf['SoftCombiner']['workerDataTimeout'] = 3.5
    hip = sc.SoftCombiner(conf, backend='hip', clock=lambda: now[0])
    host = sc.SoftCombiner(conf, backend='host', clock=lambda: now[0])
    sent = 0
    for rnd in range(max(len(c) for c in per_channel) + 3):
        for c in per_channel:
            if rnd < len(c):
                hip.insert(c[rnd])
                host.insert(c[rnd])
        a, b = hip.compareWorkers(), host.compareWorkers()
        assert len(a) == len(b)
        for da, db in zip(a, b):
            assert da.keys() == db.keys()
            for key in da:
                if key in ('data', 'trust'):
                    assert da[key].dtype == db[key].dtype and da[key].tobytes() == db[key].tobytes(), key
                else:           # statistics: equal, or both NaN (the SNR of a block of noise)
                    assert da[key] == db[key] or (da[key] != da[key] and db[key] != db[key]), key
        assert [(w.head, w.tail, w.getCount) for w in hip.workers] == [(w.head, w.tail, w.getCount) for w in host.workers]
        sent += len(a)
        now[0] += 0.3
    assert sent >= 3 and hip.host_fallbacks == 0
    hip.close()
