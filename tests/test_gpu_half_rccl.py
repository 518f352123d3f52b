"""float16 / bfloat16 over the RCCL transport in real processes
(tools/h16_check.py)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(200)
def test_half_types_two_processes():
    """2 processes on the one GPU: bf16 and fp16 SUM, allreduce_bine_bdw_remap
    and reduce_scatter_bine_permute_remap at 2 * 4099 elements, over RCCL P2P
    (literal, flat) and over the direct transport (flat: pull copies +
    k_reduce_tree for these types); every rank vs the host replay"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "h16_check.py"), "2"], env=env,
                    capture_output=True, text=True, timeout=150, ranks=2)
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert "RESULT P=2" in r.stdout
