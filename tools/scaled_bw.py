#!/usr/bin/env python3
"""Times of the scaled kernels beside the unscaled ones they must match:
  * k_reduce_tree scaled (k_reduce_tree_sc) against k_reduce_tree, 8 leaves x
    16 MiB, fp32 and bf16 -- the same bytes, one multiply per element more;
  * k_scale out of place against k_copy on the same buffers, 256 MiB fp32;
  * loopback P = 8 flat allreduce_bine_bdw_remap, fp32, 64 MiB per rank: the
    scaled call (trees scale) against the unscaled call plus a separate
    bine_scale over every rank's output, and against the unscaled call alone
    (wall clock of the whole 8-rank call: no threshold, reported).
hipEvents around each of 20 launches after 5 warm-up launches, 3 rounds per
variant, the rounds interleaved; pico-like random data (0..100), not zeros.
usage: python tools/scaled_bw.py > profiles/scaled_bw.txt
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
            print(f"  round {rnd} {k:<28} {m:10.2f} us ({lo:.2f} .. {hi:.2f}){bw}")
    b = statistics.median(med[base])
    spread = (max(med[base]) - min(med[base])) / b
    print(f"  {base}: median of rounds {b:.2f} us, spread between rounds {100 * spread:.1f} %; margin = "
          f"max(spread, 5 %) = {100 * max(spread, 0.05):.1f} %")
    for k in variants:
        if k == base:
            continue
        m = statistics.median(med[k])
        d = m / b - 1
        print(f"  {k}: median of rounds {m:.2f} us = {base} {100 * d:+.1f} %  "
              f"({'within' if d <= max(spread, 0.05) else 'OUTSIDE'} the margin)")


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    def buf(n, dt):
        return (torch.rand(n, device=dev, generator=g) * 100).to(dt)

    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed launches after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")
    # 1. the fused tree against the plain tree
    for name, tdt, dt in (("fp32", torch.float32, "float"), ("bf16", torch.bfloat16, "bfloat16")):
        n = (16 << 20) // (4 if dt == "float" else 2)
        leaves = [buf(n, tdt) for _ in range(8)]
        out = buf(n, tdt)
        assert pico_amd.reduce_tree(leaves, out, n, dt, "sum", scale=1 / 3) == 0
        compare(f"k_reduce_tree 8 leaves SUM 16 MiB/leaf, {name}",
                {"unscaled": lambda: pico_amd.reduce_tree(leaves, out, n, dt, "sum"),
                 "scaled 1/3": lambda: pico_amd.reduce_tree(leaves, out, n, dt, "sum", scale=1 / 3)},
                "unscaled", 9 * (16 << 20))
        del leaves, out
    # 2. k_scale against k_copy
    n = (256 << 20) // 4
    src, dst = buf(n, torch.float32), buf(n, torch.float32)
    compare("out of place, 256 MiB fp32",
            {"k_copy": lambda: pico_amd.copy(dst, src, n * 4),
             "k_scale 1/3": lambda: pico_amd.scale(src, dst, n, "float", 1 / 3)},
            "k_copy", 2 * (256 << 20))
    del src, dst
    # 3. fused against appended, the whole collective
    P, n = 8, (64 << 20) // 4
    comms = pico_amd.Comm.loopback(P, 0)
    for c in comms:
        c.set_flat_rs(True)
        c.set_flat_ag(2)
    sb = [buf(n, torch.float32) for _ in range(P)]
    rb = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(P)]

    def ar(scale=None):
        rc, st = pico_amd.loopback_allreduce(comms, "bine_bdw_remap", sb, rb, n, "float", "sum", scale=scale)
        assert rc == 0, st

    def appended():
        ar()
        for r in range(P):
            pico_amd.scale(rb[r], rb[r], n, "float", 1 / P)
        torch.cuda.synchronize()

    compare("loopback P = 8 flat allreduce_bine_bdw_remap, fp32, 64 MiB per rank (wall clock of the 8-rank call)",
            {"unscaled": ar, "scaled 1/P (fused)": lambda: ar(1 / P), "unscaled + bine_scale": appended},
            "unscaled", 0, timer=wall)
    for c in comms:
        c.destroy()


if __name__ == "__main__":
    main()
