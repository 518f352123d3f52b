"""k_copy's cache policy (pico_amd/csrc/kernels.hip: keep_vecs) copies the same
bytes wherever the boundary between its two kinds of loads falls.

The library reads BINE_COPY_KEEP_MIB once, so each setting runs in a fresh
child process (tools/copy_policy_check.py): copies of 0, 1, 15, 16, 17 bytes,
32 KiB - 16, 32 KiB, 32 KiB + 16 and 3 tiles + 5 bytes (a tile is 32 KiB), the
destination 0, 4 and 12 bytes past a 16-B boundary with a co-aligned source and
one pair that is not co-aligned, each inside an arena with 64 or more guard
bytes around both operands, the whole arena compared with numpy's image.

Settings: unset (the shipped policy, which gives these small copies no plain
loads), 0 (every load non-temporal), and boundaries in the middle of the first
tile (16 KiB), on a tile edge (32 KiB), beyond the end of every case (1 MiB)
and at a byte count that is no multiple of 16 (40,000 bytes, inside the second
tile).  Every setting must leave identical bytes in every arena.

These tests compare values: they cannot see which loads a tile used."""
import os
import sys
import time

import pytest

import _sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "copy_policy_check.py")
# a child imports torch, opens the GPU and makes 36 small copies: seconds; the limit only ends a hang
LIMIT = 120
SETTINGS = {
    "unset": None,
    "zero": "0",
    "mid_tile": "0.015625",               # 16 KiB
    "tile_edge": "0.03125",               # 32 KiB
    "beyond_end": "1",                    # 1 MiB > 3 tiles + 5 bytes
    "not_multiple_of_16": "0.03814697265625",   # 40,000 bytes
}
_results = {}


def child(name):
    """(returncode, sha256 of the arenas, output) of the check under SETTINGS[name], run once"""
    if name not in _results:
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("BINE_COPY_KEEP_MIB", None)
        if SETTINGS[name] is not None:
            env["BINE_COPY_KEEP_MIB"] = SETTINGS[name]
        t0 = time.time()
        r = _sub.run_kw([sys.executable, "-u", TOOL], env=env, capture_output=True, text=True, timeout=LIMIT, ranks=1)
        print(f"tools/copy_policy_check.py [{name}]: {time.time() - t0:.1f} s")
        lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x]
        res = [x for x in lines if x.startswith("RESULT ")]
        sha = res[-1].split("sha256=")[1].strip() if res else None
        _results[name] = (r.returncode, sha, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:])
    return _results[name]


@pytest.mark.timeout(LIMIT + 20)
@pytest.mark.parametrize("name", list(SETTINGS))
def test_copy_is_exact_and_writes_nowhere_else(name):
    rc, sha, out = child(name)
    print(out)
    assert rc == 0 and sha is not None, out
    assert " cases=36 bad=0 " in out, out


@pytest.mark.timeout(len(SETTINGS) * LIMIT + 20)
def test_every_setting_leaves_identical_bytes():
    shas = {name: child(name)[1] for name in SETTINGS}
    assert None not in shas.values(), shas
    assert len(set(shas.values())) == 1, shas
