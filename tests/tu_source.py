"""The host text of the library's one translation unit, for the tests that read it: ``mfbank.hip`` and the host-only parts it includes
(``*_api.hpp``, ``*_ctx.hpp``).  A later split of a part edits this file and nothing else."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pycusdr_amd', 'csrc')
UNIT = 'mfbank.hip'


def read(name):
    return open(os.path.join(CSRC, name)).read()


def included(name=UNIT):
    """The project's own headers ``name`` includes, in order (with repeats, if it has any)."""
    return re.findall(r'^\s*#\s*include\s+"([^"/]+)"', read(name), re.M)


def host_parts():
    """The host-only parts beside the unit: every ``*_api.hpp`` and ``*_ctx.hpp`` of csrc/."""
    return sorted(f for f in os.listdir(CSRC) if f.endswith(('_api.hpp', '_ctx.hpp')))


def bank_parts():
    """The bank's parts in the order the unit includes them."""
    return [f for f in included() if f.startswith('bank_')]


def host_files():
    """name -> text of the unit and every host-only part."""
    return {name: read(name) for name in [UNIT] + host_parts()}


def bank_text():
    """What used to be mfbank.hip's own text: the unit and the bank's parts, concatenated."""
    return ''.join(read(name) for name in [UNIT] + bank_parts())
