#!/usr/bin/env python3
"""Times of the 16-bit floating types' reduction kernels beside the uint16
kernels (same byte counts, same HBM streams, trivial arithmetic): k_reduce SUM
at 64 MiB per operand (out = b + a, three streams) and the 8-leaf
k_reduce_tree at 16 MiB per leaf (nine streams).  hipEvents around each of 20
launches after 5 warm-up launches; every type is measured in 3 rounds, the
rounds interleaved, so the spread between rounds of one type is the
run-to-run spread the types are compared within.
usage: python tools/h16_reduce_bw.py > profiles/h16_reduce_bw.txt
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pico_amd  # noqa: E402

TYPES = ("uint16", "float16", "bfloat16")
WARM, ITERS, ROUNDS = 5, 20, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    def buf(nbytes):   # values 0..100 of either 16-bit format are finite in the other and as uint16 anything goes
        return (torch.rand(nbytes // 2, device=dev, generator=g) * 100).to(torch.bfloat16).view(torch.int16)

    n2 = (64 << 20) // 2
    a, b, out = buf(64 << 20), buf(64 << 20), buf(64 << 20)
    n8 = (16 << 20) // 2
    leaves = [buf(16 << 20) for _ in range(8)]
    tout = buf(16 << 20)
    for dt in TYPES:
        assert pico_amd.reduce_tree(leaves, tout, n8, dt, "sum") == 0, dt
    cases = {
        "k_reduce SUM 64 MiB/operand": (lambda dt: (lambda: pico_amd.reduce3(a, b, out, n2, dt, "sum")), 3 * (64 << 20)),
        "k_reduce_tree 8 leaves SUM 16 MiB/leaf": (lambda dt: (lambda: pico_amd.reduce_tree(leaves, tout, n8, dt, "sum")),
                                                     9 * (16 << 20)),
    }
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed launches after {WARM} warm-up, {ROUNDS} rounds per "
          f"type (interleaved); us = median of a round (min .. max)")
    for name, (mk, nbytes) in cases.items():
        print(f"\n{name}  ({nbytes >> 20} MiB of HBM traffic per launch)")
        med = {dt: [] for dt in TYPES}
        for rnd in range(ROUNDS):
            for dt in TYPES:
                m, lo, hi = timed(mk(dt))
                med[dt].append(m)
                print(f"  round {rnd} {dt:<9} {m:8.2f} us ({lo:.2f} .. {hi:.2f})  {nbytes / m / 1e6:6.2f} TB/s")
        base = statistics.median(med["uint16"])
        spread = (max(med["uint16"]) - min(med["uint16"])) / base
        print(f"  uint16 median of rounds {base:.2f} us, spread between rounds {100 * spread:.1f} %; margin = "
              f"max(spread, 5 %) = {100 * max(spread, 0.05):.1f} %")
        for dt in TYPES[1:]:
            m = statistics.median(med[dt])
            d = m / base - 1
            print(f"  {dt:<9} median of rounds {m:.2f} us = uint16 {100 * d:+.1f} %  "
                  f"({'within' if d <= max(spread, 0.05) else 'OUTSIDE'} the margin)")


if __name__ == "__main__":
    main()
