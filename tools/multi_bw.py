#!/usr/bin/env python3
"""Times of the segmented copy (k_copy_segs) and of the multi-buffer allreduce
beside what they are to be compared with:
  1. one co-aligned 256 MiB segment against k_copy (bine_copy) on the same
     buffers;
  2. 64 co-aligned segments of 4 MiB (one launch) and 1,024 segments of 16 KiB
     (one call, 1,024 / 128 = 8 launches), each against that many bine_copy
     calls;
  3. 64 MiB with the source 2 bytes past a 16-B boundary and the destination on
     one (the shifted path), against bine_copy on the same pointers (which hands
     such a pair to hipMemcpyAsync) -- reported only;
  4. loopback P = 4, flat bine_bdw_remap, bfloat16 wide avg, 64 tensors of
     32 Ki and of 4 Mi elements: one allreduce_multi call against 64
     allreduce_wide calls, wall clock of the P-rank calls.
1 - 3: hipEvents around each of 20 timed calls after 5 warm-up calls, the C
entry points called with argument arrays built beforehand; 4: wall clock of 10
calls after 2.  3 rounds per variant, the rounds interleaved; every figure is
the median of a round with its (min .. max), and the spread between the rounds'
medians is printed with each comparison.  Random data, not zeros.  One GPU.
usage: python tools/multi_bw.py > profiles/multi_bw.txt
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pico_amd  # noqa: E402

WARM, ITERS, ROUNDS = 5, 20, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


def wall(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(10):
        t0 = time.perf_counter()
        fn()   # the loopback driver synchronizes every rank before it returns
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us), min(us), max(us)


def compare(title, variants, base, nbytes, timer=timed, margin=False):
    """variants: {name: fn}; `base` = the name the others are compared with;
    nbytes = bytes copied per call (read + written = twice that); margin: judge
    the others against the standing margin max(spread of base, 5 %)"""
    print(f"\n{title}")
    med = {k: [] for k in variants}
    for rnd in range(ROUNDS):
        for k, fn in variants.items():
            m, lo, hi = timer(fn)
            med[k].append(m)
            bw = f"  {nbytes / m / 1e3:8.1f} GB/s copied" if nbytes else ""
            print(f"  round {rnd} {k:<30} {m:10.2f} us ({lo:.2f} .. {hi:.2f}){bw}")
    b = statistics.median(med[base])
    spread = (max(med[base]) - min(med[base])) / b
    print(f"  {base}: median of rounds {b:.2f} us, spread between rounds {100 * spread:.1f} %")
    for k in variants:
        if k == base:
            continue
        m = statistics.median(med[k])
        sk = (max(med[k]) - min(med[k])) / m
        d = m / b - 1
        verdict = ""
        if margin:
            verdict = (f"; margin max(spread of {base}, 5 %) = {100 * max(spread, 0.05):.1f} %: "
                       f"{'within' if d <= max(spread, 0.05) else 'OUTSIDE'}")
        print(f"  {k}: median of rounds {m:.2f} us (spread {100 * sk:.1f} %) = {base} {100 * d:+.1f} %, ratio "
              f"{m / b:.3f}{verdict}")


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")

    def arrays(dst, src, nb):
        n = len(nb)
        return (n, (ctypes.c_void_p * n)(*dst), (ctypes.c_void_p * n)(*src), (ctypes.c_size_t * n)(*nb))

    def segs_fn(dst, src, nb):
        a = arrays(dst, src, nb)

        def f():
            assert L.bine_copy_segments(*a, stream) == 0
        return f

    def copies_fn(dst, src, nb):
        def f():
            for d, s, b in zip(dst, src, nb):
                L.bine_copy(d, s, b, stream)
        return f

    def case(title, nseg, seg_bytes, sphase=0):
        src = torch.randint(0, 256, (nseg * seg_bytes + 64,), dtype=torch.uint8, device=dev)
        dst = torch.zeros(nseg * seg_bytes + 64, dtype=torch.uint8, device=dev)
        sp = [src.data_ptr() + sphase + k * seg_bytes for k in range(nseg)]
        dp = [dst.data_ptr() + k * seg_bytes for k in range(nseg)]
        nb = [seg_bytes] * nseg
        segs_fn(dp, sp, nb)()
        torch.cuda.synchronize()
        assert torch.equal(dst[:nseg * seg_bytes], src[sphase:sphase + nseg * seg_bytes])
        base = f"{nseg} x bine_copy" if nseg > 1 else "k_copy (bine_copy)"
        if sphase:
            base = "bine_copy (hipMemcpyAsync)"
        compare(title, {base: copies_fn(dp, sp, nb), "k_copy_segs (one call)": segs_fn(dp, sp, nb)}, base,
                nseg * seg_bytes, margin=nseg == 1 and not sphase)
        del src, dst
        torch.cuda.empty_cache()

    case("1. one co-aligned segment of 256 MiB", 1, 256 << 20)
    case("2a. 64 co-aligned segments of 4 MiB, one launch", 64, 4 << 20)
    case("2b. 1,024 co-aligned segments of 16 KiB, one call = 8 launches", 1024, 16 << 10)
    case("3. one segment of 64 MiB, source phase 2, destination phase 0 (the shifted path; reported only)", 1,
         64 << 20, sphase=2)

    # 4. the whole collective
    P, NT = 4, 64
    comms = pico_amd.Comm.loopback(P, 0)
    for c in comms:
        c.set_flat_rs(True)
        c.set_flat_ag(2)
    for per in (32 << 10, 4 << 20):
        ts = [[(torch.rand(per, device=dev) * 100).to(torch.bfloat16) for _ in range(NT)] for _ in range(P)]

        def one():
            rc, st = pico_amd.loopback_allreduce_multi(comms, "bine_bdw_remap", None, ts, "bfloat16", "avg", wide=True)
            assert rc == 0, st

        def many():
            for k in range(NT):
                col = [ts[r][k] for r in range(P)]
                rc, st = pico_amd.loopback_allreduce_wide(comms, "bine_bdw_remap", [pico_amd.IN_PLACE] * P, col, per,
                                                          "bfloat16", "avg")
                assert rc == 0, st

        compare(f"4. loopback P = {P} flat bine_bdw_remap, bfloat16 wide avg, in place, {NT} tensors x {per >> 10} Ki "
                f"elements per rank (wall clock of the {P}-rank calls; one GPU)",
                {f"{NT} x allreduce_wide": many, "1 x allreduce_multi": one}, f"{NT} x allreduce_wide", 0, timer=wall)
        del ts
        torch.cuda.empty_cache()
    for c in comms:
        c.destroy()


if __name__ == "__main__":
    main()
