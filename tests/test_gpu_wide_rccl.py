"""Wide (binary32-accumulating) allreduce / reduce-scatter over the RCCL and
direct transports in real processes (tools/wide_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three times the measured wall time of the tool, floored at 60 s (profiles/wide_check.txt)
TIMEOUT = {2: 60, 4: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2, 4])
def test_wide_processes(P):
    """P processes on the one GPU: float16 and bfloat16, SUM times 1/P and MAX,
    allreduce_bine_bdw_remap and reduce_scatter_bine_permute_remap at 2 * 4099
    and 4 * 2048 elements, over RCCL P2P (literal: path A; flat: path B) and
    over the direct transport (flat: path B as pull copies + the wide tree),
    each case again under BINE_WIDE_TREES=0 (path A: over the direct transport
    the binary32 call's in-launch trees); every rank vs the host statement of
    the definition (tests/wide_sim.py)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "wide_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
