"""The numpy model of the device's window means (tests/snr_model.py, csrc/snr_kernels.hpp) equals numpy's own
``np.mean(np.abs(np.concatenate(pieces)))`` bit for bit -- what computeSNR (reference demodulator_base.py:635-667) takes from the
spectrum slices -- for every window length the kernel treats differently."""
import warnings

import numpy as np
import pytest

import snr_model as sm
from snr_model import LENGTHS, PAIRS


def host_mean(pieces):
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)            # "Mean of empty slice"
        return np.mean(np.abs(np.concatenate(pieces)))


def test_inputs_tell_the_orders_apart():
    """On these inputs numpy's sum is not the plain left-to-right sum at any tested length above 128, and without the 8192-element
    chunks the pairwise sum is not numpy's at some length above 8192: a model that passes below has numpy's order."""
    for n in (x for x in LENGTHS if x > 128):
        mag = np.abs(sm.sensitive(n))
        assert sm.left_to_right(mag) != np.add.reduce(mag), n

    def pairwise(v):          # one pairwise sum over the whole vector: no chunks
        if len(v) <= sm.LEAF:
            return sm.leaf_sum(v)
        n2 = len(v) // 2 - (len(v) // 2) % 8
        with np.errstate(all='ignore'):
            return sm.f32(pairwise(v[:n2]) + pairwise(v[n2:]))
    differs = 0
    for n in (8193, 8199, 8200, 16389, 1 << 15):
        mag = np.abs(sm.sensitive(n))
        differs += pairwise(mag) != np.add.reduce(mag)
    assert differs > 0


@pytest.mark.parametrize('n', LENGTHS)
def test_one_piece(n):
    x = sm.sensitive(n)
    assert sm.same_bits(sm.window_mean([x]), host_mean([x])), n


@pytest.mark.parametrize('n0,n1', PAIRS)
def test_two_pieces(n0, n1):
    x = sm.sensitive(n0 + n1, tag=1)
    pieces = [x[:n0], x[n0:]]
    assert sm.same_bits(sm.window_mean(pieces), host_mean(pieces))


@pytest.mark.parametrize('n', [5, 100, 131, 1025, 8199])
@pytest.mark.parametrize('bad', [np.inf, np.nan])
def test_inf_and_nan_elements(n, bad):
    x = sm.sensitive(n, tag=2)
    for part in ('real', 'imag'):
        y = x.copy()
        getattr(y, part)[n // 2] = bad
        got, want = sm.window_mean([y]), host_mean([y])
        assert sm.same_bits(got, want) and (np.isinf(got) if np.isinf(bad) else np.isnan(got))


def test_exact_zeros_and_all_zero_window():
    z = np.zeros(300, np.complex64)
    assert sm.same_bits(sm.window_mean([z]), host_mean([z])) and sm.window_mean([z]) == 0
    x = sm.sensitive(1000, tag=3)
    assert (x == 0).any()


def test_heap_holds_every_chunk_length():
    """The recursion of every chunk length fits the kernel's heap (at most 7 splits), and its leaves tile the chunk in order."""
    for m in range(1, sm.CHUNK + 1):
        leaves = sorted(nd for nd in sm.heap_nodes(m) if nd is not None and nd != -1)
        at = 0
        for off, ln in leaves:
            assert off == at and 0 < ln <= sm.LEAF
            at += ln
        assert at == m
