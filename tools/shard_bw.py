#!/usr/bin/env python3
"""Times of the sharded copy (k_copy_shards) and of the sharded multi-buffer
collectives beside what they are to be compared with:
  1. 8 tensors x 8 shards x 4 MiB, co-aligned, flat -> packed: one
     bine_copy_shards call against bine_copy_segments given the same 64 byte
     ranges as individual segments (judged: within max(spread, 5 %));
  2. 1,024 tensors x 8 shards x 2 KiB: bine_copy_shards (8 launches) against
     bine_copy_segments on the 8,192 ranges (its table holds 1,024 per call:
     8 calls, 64 launches) -- the ratio is reported;
  3. shape 1 with the flat side 1 byte past a 16-B boundary (the shifted path)
     -- reported only;
  4. loopback P = 4, 64 tensors with shards of 8 Ki and of 1 Mi float elements:
     one reduce_scatter_multi (bine_permute_remap) / allgather_multi (ring) call
     against 64 single calls, wall clock of the P-rank calls.
1 - 3: hipEvents around each of 20 timed calls after 5 warm-up calls, the C
entry points called with argument arrays built beforehand; 4: wall clock of 10
calls after 2.  3 rounds per variant, the rounds interleaved; every figure is
the median of a round with its (min .. max), and the spread between the rounds'
medians is printed with each comparison.  Random data, not zeros.  One GPU.
usage: python tools/shard_bw.py > profiles/shard_bw.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, compare, wall  # noqa: E402  (the same timers and report)

SEGS_PER_CALL = 1024   # BINE_MULTI_MAX


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")

    def case(title, nten, P, nb, fphase=0, margin=False):
        flat = torch.randint(0, 256, (nten * P * nb + 64,), dtype=torch.uint8, device=dev)
        packed = torch.zeros(nten * P * nb + 64, dtype=torch.uint8, device=dev)
        fp = [flat.data_ptr() + fphase + k * P * nb for k in range(nten)]
        a = (nten, P, 0, packed.data_ptr(), (ctypes.c_void_p * nten)(*fp), (ctypes.c_size_t * nten)(*([nb] * nten)))
        # the same byte ranges as individual segments, in bine_copy_segments' calls of up to 1,024
        dst = [packed.data_ptr() + j * nten * nb + k * nb for k in range(nten) for j in range(P)]
        src = [fp[k] + j * nb for k in range(nten) for j in range(P)]
        calls = []
        for i in range(0, len(dst), SEGS_PER_CALL):
            n = len(dst[i:i + SEGS_PER_CALL])
            calls.append((n, (ctypes.c_void_p * n)(*dst[i:i + n]), (ctypes.c_void_p * n)(*src[i:i + n]),
                          (ctypes.c_size_t * n)(*([nb] * n))))

        def shards():
            assert L.bine_copy_shards(*a, stream) == 0

        def segs():
            for c in calls:
                assert L.bine_copy_segments(*c, stream) == 0

        want = flat[fphase:fphase + nten * P * nb].view(nten, P, nb).transpose(0, 1).reshape(-1)
        for f in (segs, shards):
            packed.zero_()
            f()
            torch.cuda.synchronize()
            assert torch.equal(packed[:nten * P * nb], want)
        base = f"bine_copy_segments ({len(dst)} segments, {len(calls)} call{'s' if len(calls) > 1 else ''})"
        compare(title, {base: segs, "k_copy_shards (one call)": shards}, base, nten * P * nb, margin=margin)
        del flat, packed
        torch.cuda.empty_cache()

    case("1. 8 tensors x 8 shards x 4 MiB, co-aligned, one launch", 8, 8, 4 << 20, margin=True)
    case("2. 1,024 tensors x 8 shards x 2 KiB: 8 launches against 64", 1024, 8, 2 << 10)
    case("3. shape 1, flat side at phase 1, packed at phase 0 (the shifted path; reported only)", 8, 8, 4 << 20,
         fphase=1)

    # 4. the whole collectives
    P, NT = 4, 64
    comms = pico_amd.Comm.loopback(P, 0)
    for per in (8 << 10, 1 << 20):
        fulls = [[torch.rand(P * per, device=dev) * 100 for _ in range(NT)] for _ in range(P)]
        shards = [[torch.rand(per, device=dev) * 100 for _ in range(NT)] for _ in range(P)]

        def rs_one():
            rc, st = pico_amd.loopback_reduce_scatter_multi(comms, "bine_permute_remap", fulls, shards, "float", "sum")
            assert rc == 0, st

        def rs_many():
            for k in range(NT):
                rc, st = pico_amd.loopback_reduce_scatter(comms, "bine_permute_remap", [fulls[r][k] for r in range(P)],
                                                          [shards[r][k] for r in range(P)], [per] * P, "float", "sum")
                assert rc == 0, st

        def ag_one():
            rc, st = pico_amd.loopback_allgather_multi(comms, "ring", shards, fulls, "float")
            assert rc == 0, st

        def ag_many():
            for k in range(NT):
                rc, st = pico_amd.loopback_allgather(comms, "ring", [shards[r][k] for r in range(P)],
                                                     [fulls[r][k] for r in range(P)], per, "float")
                assert rc == 0, st

        what = f"{NT} tensors x {P} shards x {per >> 10} Ki float elements per rank (wall clock of the {P}-rank calls)"
        compare(f"4. loopback P = {P} reduce_scatter bine_permute_remap, float SUM, {what}",
                {f"{NT} x reduce_scatter": rs_many, "1 x reduce_scatter_multi": rs_one}, f"{NT} x reduce_scatter", 0,
                timer=wall)
        compare(f"4. loopback P = {P} allgather ring, {what}",
                {f"{NT} x allgather": ag_many, "1 x allgather_multi": ag_one}, f"{NT} x allgather", 0, timer=wall)
        del fulls, shards
        torch.cuda.empty_cache()
    for c in comms:
        c.destroy()


if __name__ == "__main__":
    main()
