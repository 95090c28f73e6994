"""The library is one translation unit, ``mfbank.hip``, whose host side stands in parts (``*_api.hpp``, ``*_ctx.hpp``) and whose kernels
stand in ``*_kernels.hpp``.  Three textual conditions keep it that way; no GPU."""
import os
import re

import tu_source

ROOT = tu_source.ROOT
HOST_TEXT = ('mfb_common.hpp', 'stage_handle.hpp')      # host-only headers that are no part but may define an entry point


def test_every_part_is_included_once_and_by_the_unit_only():
    parts = tu_source.host_parts()
    assert len(parts) == 6 + 8 and len(tu_source.bank_parts()) == 8, parts      # the six side handles, the bank's eight
    unit = tu_source.included()
    for part in parts:
        assert unit.count(part) == 1, part
    for name in os.listdir(tu_source.CSRC):
        if name != tu_source.UNIT and name.endswith(('.hpp', '.hip', '.h')):
            assert not set(tu_source.included(name)) & set(parts), name
    # the bank's parts come in dependency order, in front of the side handles', which use nothing of the bank's
    bank = [p for p in unit if p in parts and p.startswith('bank_')]
    assert bank[0] == 'bank_ctx.hpp' and bank[-1] == 'bank_debug_api.hpp'
    assert max(unit.index(p) for p in bank) < min(unit.index(p) for p in parts if not p.startswith('bank_'))


def test_every_prototype_has_one_definition():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfbank.h')).read(), flags=re.S)
    names = re.findall(r'^\s*(?:const\s+char\s*\*|int|void)\s*(mfb_\w+)\s*\(', hdr, re.M)
    assert len(names) == len(set(names)) and len(names) > 130, len(names)
    from pycusdr_amd import _lib
    assert set(_lib.PROTOTYPES) <= set(names)
    text = ''.join(tu_source.host_files().values()) + ''.join(tu_source.read(h) for h in HOST_TEXT)
    for name in names:
        assert len(re.findall(r'extern "C" [\w \*]*\b' + name + r'\(', text)) == 1, name


def test_host_files_hold_no_device_code():
    for name, text in tu_source.host_files().items():
        code = re.sub(r'//.*', '', text)
        assert not re.search(r'__global__|__device__', code), name
    # ... and no file of csrc/ is long enough to hide a seam again
    for name in os.listdir(tu_source.CSRC):
        lines = tu_source.read(name).count('\n')
        assert lines <= (300 if name == tu_source.UNIT else 1500), (name, lines)
