#!/usr/bin/env python3
"""Times of the wide (binary32-accumulating) kernels and calls beside what they
are to be compared with:
  1. k_reduce_tree_wide against the plain 16-bit k_reduce_tree of the same
     build, float16 and bfloat16, nl = 2, 4, 8, 16 leaves of 16 MiB, SUM -- both
     move (nl + 1) x 16 MiB; hipEvents around each of 20 launches after 5
     warm-up launches;
  2. allreduce_wide (bine_bdw_remap, flat forms, bfloat16 SUM times 1/P) on
     loopback ranks at P = 4 and 8, 64 Mi elements per rank: path B (the 16-bit
     plan with wide trees) against path A (BINE_WIDE_TREES=0: k_widen, the
     binary32 call, k_narrow), wall clock of the whole P-rank call, beside the
     byte model of the two paths.
3 rounds per variant, the rounds interleaved; every figure is the median of a
round with its (min .. max), and the spread between the rounds' medians is
printed with each comparison.  Pico-like random data (0..100), not zeros.
usage: python tools/wide_bw.py > profiles/wide_bw.txt
"""
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


def compare(title, variants, base, nbytes, timer=timed):
    """variants: {name: fn}; `base` = the name the others are compared with"""
    print(f"\n{title}" + (f"  ({nbytes >> 20} MiB of HBM traffic per launch)" if nbytes else ""))
    med = {k: [] for k in variants}
    for rnd in range(ROUNDS):
        for k, fn in variants.items():
            m, lo, hi = timer(fn)
            med[k].append(m)
            bw = f"  {nbytes / m / 1e6:6.2f} TB/s" if nbytes else ""
            print(f"  round {rnd} {k:<22} {m:10.2f} us ({lo:.2f} .. {hi:.2f}){bw}")
    b = statistics.median(med[base])
    spread = (max(med[base]) - min(med[base])) / b
    print(f"  {base}: median of rounds {b:.2f} us, spread between rounds {100 * spread:.1f} %")
    for k in variants:
        if k == base:
            continue
        m = statistics.median(med[k])
        sk = (max(med[k]) - min(med[k])) / m
        d = m / b - 1
        print(f"  {k}: median of rounds {m:.2f} us (spread {100 * sk:.1f} %) = {base} {100 * d:+.1f} %, ratio "
              f"{m / b:.3f}  ({'within' if abs(d) <= max(spread, sk) else 'OUTSIDE'} the run-to-run spread)")


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    def buf(n, dt):
        return (torch.rand(n, device=dev, generator=g) * 100).to(dt)

    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed launches after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")
    # 1. the wide tree against the plain 16-bit tree
    n = (16 << 20) // 2
    for name, tdt, dt in (("float16", torch.float16, "float16"), ("bfloat16", torch.bfloat16, "bfloat16")):
        for nl in (2, 4, 8, 16):
            leaves = [buf(n, tdt) for _ in range(nl)]
            out = buf(n, tdt)
            assert pico_amd.reduce_tree_wide(leaves, out, n, dt, "sum") == 0
            compare(f"tree of {nl} leaves, SUM, 16 MiB/leaf, {name}",
                    {"plain k_reduce_tree": lambda: pico_amd.reduce_tree(leaves, out, n, dt, "sum"),
                     "k_reduce_tree_wide": lambda: pico_amd.reduce_tree_wide(leaves, out, n, dt, "sum")},
                    "plain k_reduce_tree", (nl + 1) * (16 << 20))
            del leaves, out
    # 2. path B against path A, the whole collective
    n = 64 << 20
    for P in (4, 8):
        comms = pico_amd.Comm.loopback(P, 0)
        for c in comms:
            c.set_flat_rs(True)
            c.set_flat_ag(2)
        sb = [buf(n, torch.bfloat16) for _ in range(P)]
        rb = [torch.empty(n, dtype=torch.bfloat16, device=dev) for _ in range(P)]
        assert pico_amd.wide_plan("allreduce", "bine_bdw_remap", P, count=n, flat_ag=2, flat_rs=True)

        def ar(trees):
            if trees:
                os.environ.pop("BINE_WIDE_TREES", None)
            else:
                os.environ["BINE_WIDE_TREES"] = "0"
            rc, st = pico_amd.loopback_allreduce_wide(comms, "bine_bdw_remap", sb, rb, n, "bfloat16", "sum",
                                                      scale=1 / P)
            assert rc == 0, st

        # per rank and element: exchanged bytes (reduce-scatter + allgather, (P-1)/P of the buffer each way)
        # and HBM bytes of the conversion passes (k_widen 2 + 4, k_narrow 4 + 2)
        f = 2 * (P - 1) / P
        print(f"\nbyte model, P = {P}, per rank and element: path B sends {2 * f:.2f} B; path A sends {4 * f:.2f} B "
              f"and converts 12 B through HBM")
        compare(f"loopback P = {P} flat allreduce_wide bine_bdw_remap, bfloat16 SUM x 1/P, 64 Mi elements per rank "
                f"(wall clock of the {P}-rank call)",
                {"path A (through binary32)": lambda: ar(False), "path B (wide trees)": lambda: ar(True)},
                "path A (through binary32)", 0, timer=wall)
        os.environ.pop("BINE_WIDE_TREES", None)
        for c in comms:
            c.destroy()
        del sb, rb, comms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
