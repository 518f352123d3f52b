"""Multi-buffer allreduce over the RCCL and direct transports in real processes
(tools/multi_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three times the measured wall time of the tool, floored at 60 s (profiles/multi_check.txt)
TIMEOUT = {2: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2])
def test_multi_processes(P):
    """P processes on the one GPU: the seven-tensor list, float SUM and bfloat16
    wide avg, allreduce_bine_bdw_remap out of place and in place, over RCCL P2P
    (literal and flat) and over the direct transport (flat); every rank vs the
    host statement of the single call on the concatenation"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "multi_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
