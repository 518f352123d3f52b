"""Scaled allreduce / reduce-scatter over the RCCL and direct transports in
real processes (tools/scaled_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(200)
def test_scaled_two_processes():
    """2 processes on the one GPU: fp32 and bf16 SUM times 1/3,
    allreduce_bine_bdw_remap and reduce_scatter_bine_permute_remap at 2 * 4099
    elements, over RCCL P2P (literal: trailing scale; flat: the flagged trees
    scale) and over the direct transport (flat: fp32 in-launch trees + a
    trailing scale, bf16 pull copies + the scaled tree); the RCCL flat form in
    graph mode with two scales on the same buffers; every rank vs S(host
    replay of the literal unscaled plan)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "scaled_check.py"), "2"], env=env,
                    capture_output=True, text=True, timeout=150, ranks=2)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x or "graph" in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert "RESULT P=2" in r.stdout
