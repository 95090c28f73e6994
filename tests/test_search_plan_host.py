"""The segment search's planner (pycusdr_amd/csrc/search_plan.hpp) without a device: mfb_debug_search_plan with no handle plans a
set of inputs on the host.  tests/golden/search_plans.json.xz (compressed JSON) holds the plan of every case -- banks named for the branch they reach x
block lengths x bins x blocks a launch x CUs, and each environment switch and tuning singly against the defaults -- recorded from
the planner as it stood inside mfbank.hip (the fixture names the commit).  Every field of every case must come out equal: they are
integers, there is no tolerance."""
import json
import lzma
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pycusdr_amd', 'csrc')


@pytest.fixture(scope='module')
def fixture():
    import __graft_entry__
    __graft_entry__.build()
    with lzma.open(os.path.join(ROOT, 'tests', 'golden', 'search_plans.json.xz'), 'rt') as f:
        return json.load(f)


def _cases(fx):
    """(label, inputs, nb, recorded plan as a dict | None where the library refuses), in the fixture's order"""
    fields, groups = fx['plan_fields'], fx['groups']
    for sw, recorded in zip(fx['switches'], fx['cases']):
        it = iter(recorded)
        for bank in fx['banks']:
            base = dict(fx['defaults'], **{k: v for k, v in bank.items() if k != 'name'})
            base.update(sw['set'])
            for l2 in sw['log2N']:
                for d in sw['Dtot']:
                    for cus in fx['num_cus']:
                        for nb in fx['nb']:
                            idx = next(it)
                            plan = None
                            if idx >= 0:
                                plan = {}
                                for k, (g, (a, b)) in enumerate(groups.items()):          # (plans and tables are stored by column)
                                    row = fx['plans'][k][idx]
                                    plan.update(zip(fields[a:b], (col[row] for col in fx['tables'][g])))
                            yield (sw['name'], bank['name'], l2, d, cus, nb), dict(base, N=1 << l2, Dtot=d, num_cus=cus), nb, plan
        assert next(it, None) is None, sw['name']


def test_every_recorded_case_plans_as_recorded(fixture):
    from pycusdr_amd.mfbank import debug_search_plan
    n, refused, wrong = 0, 0, []
    for label, inputs, nb, want in _cases(fixture):
        n += 1
        try:
            got = debug_search_plan(inputs, nb)[1]
        except ValueError:
            got = None
        refused += got is None
        if got != want and len(wrong) < 10:
            wrong.append((label, {k: (got[k], want[k]) for k in want if got[k] != want[k]} if got and want else (got, want)))
    assert not wrong, wrong
    # the whole product the fixture promises, none left out: 24 banks x 9 (CUs, blocks) x (5 x 16 + 12 switch rows x 3 x 4)
    assert n == 24 * 9 * (5 * 16 + 12 * 3 * 4) and 0 < refused < n // 10


def test_the_fixture_reaches_every_form_and_every_branch_it_names(fixture):
    plans = {label: p for label, _, _, p in _cases(fixture) if label[0] == 'defaults' and label[3:] == (256, 256, 1)}
    form = lambda bank, l2: plans[('defaults', bank, l2, 256, 256, 1)]['form']       # noqa: E731
    assert [form(f'T{T}', 18) for T in (33, 34, 48, 49)] == [2, 4, 4, 2]               # the wrap_kt edges
    assert form('T48', 17) == 2                                                      # ... and k_segw from 2^18 samples only
    assert [form(b, 18) for b in ('T48_per_filter', 'T48_nonuniform_MU7', 'T48_span_MB3', 'T80_M16')] == [2, 2, 4, 2]
    assert [form(b, 18) for b in ('T384_MU8', 'T384_MU9')] == [3, 1]                 # 2048 points: filter side for up to 8 rows
    assert plans[('defaults', 'T80_M16', 18, 256, 256, 1)]['fb'] == 8
    assert plans[('defaults', 'T4097_auto', 18, 256, 256, 1)]['path'] == 1 and plans[('defaults', 'T4097_segment', 18, 256, 256, 1)]['segl'] == 13
    assert plans[('defaults', 'T2050_segment', 13, 256, 256, 1)] is None             # no room for segments: refused, not planned
    assert {p['sumq'] for p in plans.values() if p} == {0, 1, 2}


def test_the_rule_restated_for_the_device_agrees_with_the_plan_over_the_whole_table(fixture):
    """planned_bins of tests/test_gpu_wrap_wide.py -- the independent restatement the device is held to -- against the plan's fb on
    every matrix-core row of the 8-filter, 48-tap bank: all bins, all CU counts, 2^18 and 2^20 samples, one block, default switches."""
    from test_gpu_wrap_wide import planned_bins
    n = 0
    for label, _, nb, plan in _cases(fixture):
        sw, bank, l2, d, cus, _ = label
        if sw == 'defaults' and bank == 'T48' and l2 in (18, 20) and nb == 1:
            assert plan['form'] == 4 and plan['nfull'] >= 64
            assert planned_bins(d, cus, plan['nfull']) == plan['fb'], label
            n += 1
    assert n == 2 * 16 * 3


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_each_decision_is_written_once():
    import tu_source
    hip, plan = tu_source.bank_text(), _src('search_plan.hpp')      # (mfbank.hip and the bank's parts: what used to be mfbank.hip)
    both = hip + plan
    assert both.count('(size_t)in.Dtot * MU * 16384 <= ((size_t)256 << 20)') == 1 and '* 16384 <=' not in hip       # the filter-side predicate
    assert both.count('span || in.uniform_mult') == 1 and hip.count('std::all_of(c->h_mult') == 1              # the presum test
    for var in ('MFB_SEG_FSM', 'MFB_SEG_WRAP_MFMA', 'MFB_SEG_FSM_RECT', 'MFB_SEG_FSM_GROUP'):
        assert both.count(f'getenv("{var}")') == 1 and f'getenv("{var}")' in plan, var
    assert 'fsm_fb' not in both and 'fsm_fs' not in both
    for name in ('seg_cost', 'plan_seg', 'fsm_plan', 'wrap_kt'):
        assert not re.search(rf'\b{name}\b', hip), name
    # the planner is host arithmetic: no HIP runtime call, no handle
    code = re.sub(r'//.*', '', plan)
    assert not re.search(r'\bhip[A-Z]\w*\s*\(|\bmfb_ctx\b', code)
