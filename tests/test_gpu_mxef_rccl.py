"""The MX-quantized gradient reduce-scatter with an error-feedback residual over the
RCCL and direct transports in real processes, graph mode included
(tools/mxef_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tools/mxrs_check.py's limit: the same forms, the same process start-up
TIMEOUT = {2: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2])
def test_mxef_processes(P):
    """P processes on the one GPU, the gradients of six tensors and their
    residuals each: mx_reduce_scatter_multi_ef twice (float through e4m3,
    bfloat16 through e2m1 averaged), the second call carrying the first one's
    residuals, over RCCL P2P (literal and flat) and over the direct transport,
    then twice in graph mode; every rank's shards and residuals vs
    tests/mxef_sim.py over all ranks' gradients"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    # 4 HW queues per rank, HIP's default: with fewer, graph mode keeps a call that
    # makes RCCL calls eager and the tool's replay case would have nothing to replay
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "mxef_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P, queues=4)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
