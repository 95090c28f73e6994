"""The channeliser's launch plan (pycusdr_amd/csrc/channelize_plan.hpp -- the one place libmfbank states it) without a device: a
stand-alone program (tests/csrc/channelize_plan_print.cpp, plain C++, no HIP) prints the ChzGeom, the grid and the input span of
every (kind, U, D, T, M, out_base, out_count, cell_frames) of tests/golden/channelize_plans.json, which was recorded from the
helpers as they stood in the four kernel headers and from the formulas of mfbank.hip, before ChzGeom was built on them (the
fixture names the commit).  Every field of every row must come out equal: they are integers, there is no tolerance."""
import json
import os
import re
import shutil
import subprocess

import pytest

import edge_shapes as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pycusdr_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'csrc', 'channelize_plan_print.cpp')
INTEGER, RATIONAL, UNIFORM, SURVEY = range(4)


def golden():
    """the fixture's rows as dicts, in its order"""
    with open(os.path.join(ROOT, 'tests', 'golden', 'channelize_plans.json')) as f:
        fx = json.load(f)
    return fx, [dict(zip(fx['fields'], row)) for row in fx['rows']]


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    fx, rows = golden()
    exe = tmp_path_factory.mktemp('channelize_plan') / 'channelize_plan_print'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', SRC, '-o', str(exe)], capture_output=True,
                           text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)] + [':'.join(str(r[k]) for k in fx['inputs']) for r in rows], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    got = [{k: int(v) for k, v in (kv.split('=') for kv in line.split())} for line in run.stdout.strip().splitlines()]
    assert len(got) == len(rows)
    return rows, got


def test_every_recorded_plan_is_reproduced(printed):
    rows, got = printed
    wrong = [(w, {k: (g[k], w[k]) for k in w if g[k] != w[k]}) for w, g in zip(rows, got) if g != w]
    assert not wrong, wrong[:10]


def test_the_fixture_covers_what_it_promises():
    _, rows = golden()
    of = lambda kind: [r for r in rows if r['kind'] == kind]                             # noqa: E731
    shapes = {(r['D'], r['T']) for r in of(INTEGER)}
    assert {(s[0], s[1]) for s in es.CHZ_SHAPES} | {(2, 1), (64, 1024)} <= shapes
    # the D on either side of each width change at T = 1024, by the independent restatement
    for D in range(3, es.CHZ_MAX_DECIM + 1):
        if es.chz_threads(D, 1024) != es.chz_threads(D - 1, 1024):
            assert {(D - 1, 1024), (D, 1024)} <= shapes, D
    assert {r['threads'] for r in of(INTEGER)} == {64, 128, 256} == {r['threads'] for r in of(RATIONAL)}
    ratios = {(r['U'], r['D']) for r in of(RATIONAL)}
    assert ratios == {(1, 2), (1, 63), (1, 64), (2, 3), (2, 63), (3, 4), (3, 64), (31, 32), (31, 63), (31, 64), (32, 33), (32, 63)}
    assert all({r['T'] for r in of(RATIONAL) if (r['U'], r['D']) == ud} == {ud[0], 67, 1024} for ud in ratios)
    plans = {(M, D, T) for M in (8, 16, 32, 64, 128, 256) for D in (2, M // 2, M) for T in (1, M, 257, 2049, 4096)}
    assert {(r['M'], r['D'], r['T']) for r in of(UNIFORM)} == plans == {(r['M'], r['D'], r['T']) for r in of(SURVEY)}
    for M, D, T in plans:                                  # the survey's cells around its frames per workgroup: C takes both branches
        mine = [r for r in of(SURVEY) if (r['M'], r['D'], r['T']) == (M, D, T)]
        Fs = mine[0]['tile']
        assert {r['cell_frames'] for r in mine} == {max(4, c) for c in (4, Fs // 2, Fs, 2 * Fs, 65536)}
        assert {r['C'] == r['cell_frames'] for r in mine} == {True, False}


def test_the_integer_plans_equal_the_restatement_of_edge_shapes():
    """tests/edge_shapes.py restates chz_threads and chz_row_len in Python, independently of the package"""
    _, rows = golden()
    n = 0
    for r in rows:
        if r['kind'] == INTEGER:
            w = es.chz_threads(r['D'], r['T'])
            assert (r['threads'], r['tile'], r['L']) == (w, w, es.chz_row_len(w, r['D'], r['T'])), r
            assert r['lds_bytes'] == r['D'] * r['L'] * 8 <= es.CHZ_LDS_BUDGET
            n += 1
    assert n >= 2 * len({(s[0], s[1]) for s in es.CHZ_SHAPES})


MOVED_HELPERS = ('chz_row_len', 'chz_threads', 'chzr_branch_taps', 'chzr_span', 'chzr_row_len', 'chzr_threads', 'chu_lds_bytes', 'chu_frames',
                 'chus_lds_bytes', 'chus_frames')
MOVED_LIMITS = ('CHZ_MAX_CHANNELS', 'CHZ_MAX_DECIM', 'CHZ_MAX_TAPS', 'CHZ_MAX_THREADS', 'CHZ_LDS_BUDGET', 'CHZ_MAX_IN', 'CHZ_MAX_OUT',
                'CHZR_MAX_INTERP', 'CHU_THREADS', 'CHU_MAX_BINS', 'CHU_MAX_TAPS', 'CHU_LDS_BUDGET', 'CHU_MAX_SET', 'CHUS_MIN_LOG2',
                'CHUS_MAX_LOG2', 'CHUS_MAX_TABLE', 'CHUS_SCRATCH')


def test_each_helper_and_limit_is_defined_once():
    src = lambda name: open(os.path.join(CSRC, name)).read()                             # noqa: E731
    plan = src('channelize_plan.hpp')
    import tu_source
    others = {name: src(name) for name in ('mfbank.hip', 'channelize_api.hpp', 'synthesize_uniform_api.hpp', 'channelize_kernels.hpp',
                                           'channelize_rational_kernels.hpp', 'channelize_uniform_kernels.hpp',
                                           'channelize_survey_kernels.hpp', *tu_source.bank_parts())}
    assert len(tu_source.bank_parts()) >= 8                 # (all code that stood in mfbank.hip is still among the others)
    for name in MOVED_HELPERS:
        define = rf'^[ \w]*\b{name}\s*\([^;]*\)\s*\{{'                                   # a function's head, at the start of a line
        assert len(re.findall(define, plan, re.M)) == 1, name
        assert not any(re.search(define, text, re.M) for text in others.values()), name
    for name in MOVED_LIMITS:
        define = rf'^\s*#\s*define\s+{name}\b'
        assert len(re.findall(define, plan, re.M)) == 1, name
        assert not any(re.search(define, text, re.M) for text in others.values()), name
    # the handle states its plan as a ChzGeom, not as a pair of booleans
    hip = others['channelize_api.hpp']                      # (the channeliser's host side: a part of mfbank.hip's translation unit)
    handle = hip[hip.index('struct mfb_channelizer '):]
    handle = handle[:handle.index('\n};')]
    assert 'ChzGeom plan' in handle and not re.search(r'\bbool\b[^;]*\b(uniform|rational)\b', handle)
    # the plan is host arithmetic: no HIP header, no runtime call, no handle
    code = re.sub(r'//.*', '', plan)
    assert not re.search(r'hip_runtime|\bhip[A-Z]\w*\s*\(|\bmfb_channelizer\b|__global__|__device__', code)
