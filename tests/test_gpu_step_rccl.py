"""Dynamic loss scaling over the RCCL and direct transports in real processes,
graph mode included (tools/step_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three times the measured wall time of the tool, floored at 60 s (profiles/step_check.txt)
TIMEOUT = {2: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2])
def test_step_processes(P):
    """P processes on the one GPU, the shards of seven tensors each: norm_multi,
    step_update and adamw_multi_dyn (float16, ring) over RCCL P2P (literal and
    flat) and over the direct transport, one taken and one skipped step each (an
    inf on the last rank alone), then the taken step twice in graph mode; every
    rank's state vs the numpy statement and vs the other ranks', p', m', v' and
    params vs the sim, and nothing but the state changed by a skipped step"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    # 4 HW queues per rank, HIP's default: with fewer, graph mode keeps a call that
    # makes RCCL calls eager and the tool's replay case would have nothing to replay
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "step_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P, queues=4)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
