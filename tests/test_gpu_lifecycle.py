"""Ownership: every device buffer, pinned buffer, stream and event of the library is held by an owner that releases it
(mcx_engine_internal.hpp), and mcx_debug_live_resources counts what the owners hold.  One fresh child process
(tests/lifecycle_worker.py) runs every kind of engine and every stand-alone entry point at its smallest shape and finds the
count at (0, 0, 0, 0) after each close -- and the category a scenario is about above zero before it, so that a scenario
which no longer reaches its lazily created resources fails.  The Murray scenario reaches the chunked sweep (its stream and
events are asserted): 8192 chains of 16 parameters, the fewest a pass is cut into column chunks for."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_engine_store_and_call_gives_everything_back():
    r = subprocess.run([sys.executable, os.path.join(HERE, "lifecycle_worker.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    if r.returncode != 0:
        print(out)
    assert r.returncode == 0, "the lifecycle worker ended with status %d" % r.returncode
    assert "lifecycle: all scenarios done" in out
