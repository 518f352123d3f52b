"""Sharded multi-buffer reduce-scatter and allgather over the RCCL and direct
transports in real processes, graph mode included (tools/shard_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three times the measured wall time of the tool, floored at 60 s (profiles/shard_check.txt)
TIMEOUT = {2: 60}


@pytest.mark.timeout(200)
@pytest.mark.parametrize("P", [2])
def test_shard_processes(P):
    """P processes on the one GPU: the seven-tensor list, reduce_scatter_multi
    (float SUM and bfloat16 wide avg; out of place and rbufs inside sbufs) and
    allgather_multi (float and bfloat16; out of place and in place) over RCCL P2P
    (literal and flat) and over the direct transport (flat), then both in graph
    mode; every rank vs the host statement (the oracle, tests/wide_sim.py,
    concatenation)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    # 4 HW queues per rank, HIP's default: with fewer, graph mode keeps a call that
    # makes RCCL calls eager (executor.cpp, multi_branch_graphs_ok) and the tool's
    # replay cases would have nothing to replay
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "shard_check.py"), str(P)], env=env,
                    capture_output=True, text=True, timeout=TIMEOUT[P], ranks=P, queues=4)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P}" in r.stdout
