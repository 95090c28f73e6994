"""The byte layout of a block's result record (pycusdr_amd/csrc/record_layout.hpp -- the one place libmfbank states it) against
the formulas the record has had since the batch path exists, restated here independently: a stand-alone program
(tests/csrc/record_layout_print.cpp, plain C++, no HIP) prints every offset for a handful of (band capacity, symbols, stages)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'record_layout_print.cpp')

# the sizes the layout depends on, as bank_ctx.hpp / stream_kernels.hpp define them (the program takes them on its command line)
HEAD, POST_MAX, END_MAX, MAX_TMPL, MAX_HITS, EDGE_CANDS = 256, 512, 32, 2, 64, 4
EDGE_BYTES = 4 * (1 + 1 + 2 + 2 * 8 + 2 * 8)        # StreamEdge: a_rel, valid, n[2], idx[2][8], score[2][8], int32 each
CONSTS = [HEAD, POST_MAX, END_MAX, MAX_TMPL, MAX_HITS, EDGE_CANDS, EDGE_BYTES]

# band capacity 0, odd and even; symbol counts around a multiple of 16, where align16(n) (the byte arrays) and align16(4 n) (the
# int arrays) round differently; a realistic count; stages off and on
TRIPLES = [(bcap, n, st) for bcap in (0, 7, 1024) for n in (1, 15, 16, 17, 2341) for st in (0, 1)]
ORDER = ['scalars', 'bands', 'sym', 'cen', 'mag', 'bits', 'cenw', 'trust', 'post', 'end', 'hits', 'edges']


def align16(x):
    return (x + 15) // 16 * 16


def expected(bcap, n, stages):
    """offsets and sizes, field by field: head 256, bands align16(2 bcap 8), three arrays of align16(4 n); with stages
    3 x align16(n), post, end, hits, edges"""
    sizes = [('scalars', HEAD), ('bands', align16(2 * bcap * 8)), ('sym', align16(4 * n)), ('cen', align16(4 * n)), ('mag', align16(4 * n))]
    if stages:
        sizes += [('bits', align16(n)), ('cenw', align16(n)), ('trust', align16(n)), ('post', POST_MAX), ('end', END_MAX),
                  ('hits', MAX_TMPL * 2 * MAX_HITS * 4), ('edges', align16(EDGE_CANDS * EDGE_BYTES))]
    off, at = {}, 0
    for name, size in sizes:
        off[name] = at
        at += size
    core = HEAD + align16(2 * bcap * 8) + 3 * align16(4 * n)
    return off, dict(sizes), core, at


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path_factory.mktemp('record_layout') / 'record_layout_print'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', SRC, '-o', str(exe)], capture_output=True,
                           text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)] + [str(v) for v in CONSTS] + [f'{b}:{n}:{s}' for b, n, s in TRIPLES], capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    rows = [{k: int(v) for k, v in (kv.split('=') for kv in line.split())} for line in run.stdout.strip().splitlines()]
    assert len(rows) == len(TRIPLES)
    return rows


@pytest.mark.parametrize('i', range(len(TRIPLES)), ids=[f'bcap{b}-n{n}-stages{s}' for b, n, s in TRIPLES])
def test_layout_equals_the_restated_formulas(printed, i):
    bcap, n, stages = TRIPLES[i]
    got = printed[i]
    assert (got['bcap'], got['symbols'], got['stages']) == (bcap, n, stages)
    off, sizes, core, total = expected(bcap, n, stages)
    for name in ORDER:
        assert got[name] == off.get(name, 0), (name, got, off)          # (the stage fields are 0 without stages)
    assert got['core'] == core and got['bytes'] == total, (got, core, total)
    if stages:
        assert got['bits'] == core
    else:
        assert got['bytes'] == core
    # increasing, 16-byte aligned, and the record ends where its last field does
    present = [name for name in ORDER if name in off]
    offs = [got[name] for name in present]
    assert offs[0] == 0 and all(a <= b for a, b in zip(offs, offs[1:])), offs
    assert all(a < b for a, b, name in zip(offs, offs[1:], present) if sizes[name] > 0), offs
    assert all(o % 16 == 0 for o in offs) and got['bytes'] % 16 == 0, offs
    assert got['bytes'] == offs[-1] + sizes[present[-1]]
