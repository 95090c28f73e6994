"""The scene of the survey tests (test_channelizer_survey_host.py, test_gpu_channelizer_survey.py): unit-variance noise over the
whole capture, a tone on bin 3 through the cells 2..5 and a tone on bin -5 through cell 4, at M = 16, D = 8, T = 129, L = 32.

A tone is switched on T - 1 input samples before its first cell, so that every frame of its cells reads nothing but tone, and off
with the last frame of its last cell.  The filter is T - 1 = 16 frames long: the half-filled frames fall into the cell before the
first and the cell behind the last, the one transition cell at each edge, about which the scene says nothing.  A bin next to a
tone receives it through the taps' transition band: ``adjacent`` names those bins from the taps' response."""
import numpy as np

from pycusdr_amd.channelizer import design_taps

FS = 1.024e6
M, D, L, NCELLS = 16, 8, 32, 8
TAPS = design_taps(D)                      # T = 129
THRESHOLD = 4.0
AMPLITUDE = 2.0                            # |H(0)| = 1: 4.0 per frame in the tone's bin against sum h^2 = 0.092 of the noise
TONES = ((3, 2, 5), (-5, 4, 4))            # (bin, first cell, last cell)
STOP_BAND = 1e-6                           # |H|^2 below this is the taps' stop band (a Kaiser window of beta 8: 80 dB and more)


def response(offset_bins):
    """|H|^2 of the taps at ``offset_bins / M`` cycles per input sample from a bin's centre."""
    t = np.arange(len(TAPS))
    return float(np.abs(np.sum(TAPS.astype(np.float64) * np.exp(-2j * np.pi * offset_bins / M * t))) ** 2)


def adjacent(b):
    """The bins other than ``b`` whose centre a tone on ``b`` reaches outside the taps' stop band."""
    return sorted((b + j) % M for j in range(1, M) if response(j) > STOP_BAND)


def capture(in_count, seed=11):
    """complex64 [in_count] from position 0."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal(in_count) + 1j * rs.standard_normal(in_count)) / np.sqrt(2.0)
    n = np.arange(in_count)
    for b, first, last in TONES:
        on = (n >= first * L * D - (len(TAPS) - 1)) & (n < (last + 1) * L * D)
        x = x + on * AMPLITUDE * np.exp(2j * np.pi * ((b % M) / M) * n)
    return x.astype(np.complex64)


def expectation():
    """(occupied, judged) bool [NCELLS][M]: the scene's occupancy, and the cells it speaks about -- all but the transition cells of a
    tone's bin and of the bins adjacent to it, and but the adjacent bins throughout the tone."""
    occupied = np.zeros((NCELLS, M), dtype=bool)
    judged = np.ones((NCELLS, M), dtype=bool)
    for b, first, last in TONES:
        occupied[first:last + 1, b % M] = True
        near = adjacent(b % M)
        for k in [b % M] + near:
            for s in (first - 1, last + 1):
                if 0 <= s < NCELLS:
                    judged[s, k] = False
        judged[first:last + 1, near] = False
    return occupied, judged
