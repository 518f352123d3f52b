"""Global norm and clipping over the RCCL and direct transports in real
processes, graph mode included (tools/norm_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three times the measured wall time of the tool, floored at 60 s (profiles/norm_check.txt)
TIMEOUT = {2: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2])
def test_norm_processes(P):
    """P processes on the one GPU, seven tensors whose counts differ per rank:
    norm_multi and clip_multi (float and bfloat16, bine_lat) over RCCL P2P
    (literal and flat) and over the direct transport, then norm_multi in graph
    mode; every rank vs the host statement (the oracle's allreduce of the
    ranks' sum-of-squares vectors, numpy's coefficient, bine_scale)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    # 4 HW queues per rank, HIP's default: with fewer, graph mode keeps a call that
    # makes RCCL calls eager and the tool's replay case would have nothing to replay
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "norm_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P, queues=4)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
