#!/usr/bin/env python3
"""bine_copy (k_copy) under one setting of BINE_COPY_KEEP_MIB.  The library
reads the variable once, at its first copy, so every setting needs a process of
its own (tests/test_gpu_copy_policy.py starts one per setting):

    BINE_COPY_KEEP_MIB=0.015625 python tools/copy_policy_check.py

With the variable set the policy applies to copies of every size, which brings
the boundary between the two kinds of loads down to a few tiles.  Cases: copies
of 0, 1, 15, 16, 17 bytes, 32 KiB - 16, 32 KiB, 32 KiB + 16 (a tile is 32 KiB)
and 3 tiles + 5 bytes, each with the destination 0, 4 and 12 bytes past a 16-B
boundary and the source co-aligned with it, and once with a source that is not
(the runtime's copy: the variable must change nothing).  Both operands lie in
one arena of random bytes with 64 or more guard bytes around each; after the
copy the whole arena is compared with numpy's image of it.  Prints one RESULT
line with the sha256 of all arenas read back from the device; exits non-zero
on a mismatch, after naming the case and the first differing byte."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE = 32768          # kBlock * kCopyU vectors of 16 bytes
GUARD = 64
SIZES = (0, 1, 15, 16, 17, TILE - 16, TILE, TILE + 16, 3 * TILE + 5)
# (destination phase, source phase) mod 16
PHASES = ((0, 0), (4, 4), (12, 12), (0, 2))


def layout(n, dphase, sphase):
    """(source offset, destination offset, arena bytes): offsets from a 256-B
    aligned base, each operand at its phase with GUARD or more bytes around it"""
    src = GUARD + sphase
    dst = (src + n + GUARD + 15) // 16 * 16 + dphase
    return src, dst, dst + n + GUARD


def cases():
    return [(n, d, s) for n in SIZES for d, s in PHASES]


def main():
    import torch

    import pico_amd
    assert torch.cuda.is_available(), "needs an MI355X"
    L = pico_amd.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(4242)
    h = hashlib.sha256()
    bad = 0
    for n, dphase, sphase in cases():
        src, dst, total = layout(n, dphase, sphase)
        img = rng.integers(0, 256, size=total, dtype=np.uint8)
        want = img.copy()
        want[dst:dst + n] = img[src:src + n]
        arena = torch.from_numpy(img).to(dev)
        base = arena.data_ptr()
        assert base % 256 == 0 and (base + dst) % 16 == dphase and (base + src) % 16 == sphase
        rc = L.bine_copy(base + dst, base + src, n, stream)
        torch.cuda.synchronize()
        got = arena.cpu().numpy()
        h.update(got.tobytes())
        if rc != 0 or not np.array_equal(got, want):
            bad += 1
            at = int(np.flatnonzero(got != want)[0]) if rc == 0 else -1
            print(f"MISMATCH n={n} dst phase {dphase} src phase {sphase} rc={rc}: first differing byte {at} "
                  f"(source at {src}, destination at {dst}, arena {total})", flush=True)
    print(f"RESULT keep_mib={os.environ.get('BINE_COPY_KEEP_MIB')} cases={len(cases())} bad={bad} "
          f"sha256={h.hexdigest()}", flush=True)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
