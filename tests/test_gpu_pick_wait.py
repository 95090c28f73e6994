"""The host takes a pick from the handle's page-locked slot when it arrives (read_pick in csrc/bank_search_api.hpp; k_pick stores {two floats, the
pick's number, a check word} in one 16-byte store) and no longer waits for the stream to drain.  What could go wrong is a pick that is
not this call's: the slot still holding the pick before.  So two resident 2^15-sample blocks whose carriers lie 20 bins apart alternate
through 300 find_carrier calls on one handle, and through 300 each on two handles in two threads; pick and pick_column on a device
table run between two find_carrier calls; and get_scores right behind a find_carrier must return the table that pick was made on.
Every result must be the bits of that block's (or table's) own pick, taken once with the table read back behind it and held to the
oracle's scan of that table.  The assertions are in tests/children/pick_wait_child.py; each mode runs in a child under a timeout, so
that a wait that never ends is a failure here and not a hang."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'children', 'pick_wait_child.py')


@pytest.mark.parametrize('mode', ['alternate', 'threads', 'between'])
def test_every_pick_is_this_calls_pick(mode):
    r = subprocess.run([sys.executable, CHILD, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith(f'ok {mode}')
