"""The threshold and boundary arithmetic of launch_copy's cache policy
(pico_amd/csrc/bine_internal.h: copy_keep_policy, copy_keep_vecs) on the CPU:
tools/copy_policy_plan.cpp built with g++ and the host sanitizers.  keep_vecs
never exceeds the copy's whole vectors, is 0 below the size threshold, and
BINE_COPY_KEEP_MIB parses to the bytes it names (junk: the defaults)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pico_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "copy_policy_plan.cpp")
EXE = os.path.join(ROOT, "tools", "_build", "copy_policy_plan")


def test_keep_vecs_stays_within_the_copy_and_is_zero_below_the_threshold():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    deps = [SRC, os.path.join(CSRC, "bine_internal.h"), os.path.join(ROOT, "include", "bine_amd.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bad=0" in r.stdout, r.stdout[-3000:]
