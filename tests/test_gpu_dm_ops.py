"""The direct peer-memory transport's own reductions in real processes:
k_dm_fused<T, OP> and k_dm_move_tree<T, OP, NL> on all six element types and
four ops, at the vector counts where their slices and guarded tiles can go
wrong, with NaN / inf / signed zeros / denormals, the types' extremes and
top-bit values planted, every rank's output byte for byte against the oracle,
the bytes past each output untouched, and every call's form asserted
(tools/dm_ops_check.py; its table is proved on the CPU by
tests/test_dm_ops_cases.py).  P ranks share the test box's one GPU.  The
timeouts are three times the measured wall times, floored at 60 s
(profiles/dm_ops_check.txt)."""
import os
import sys

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (P, mode, the subprocess's timeout in seconds)
RUNS = ((2, "small", 60), (2, "large", 60), (4, "small", 60), (4, "large", 60), (8, "large", 60), (3, "large", 60))


@pytest.mark.parametrize("P,mode,limit", [pytest.param(P, m, t, marks=pytest.mark.timeout(t + 20), id=f"{P}-{m}")
                                          for P, m, t in RUNS])
def test_direct_transport_reductions_every_type_and_op(P, mode, limit):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "dm_ops_check.py"), str(P), mode], env=env,
                    capture_output=True, text=True, timeout=limit, ranks=P)
    bad = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x or " ok, " in x]
    assert r.returncode == 0, "\n".join(bad[:40]) + "\n" + r.stderr[-2000:]
    assert f"RESULT P={P} mode={mode}" in r.stdout
