#!/usr/bin/env python3
"""Times of the MX block-scaled quantization kernel beside kernels it is to be
compared with, one 64 Mi-element float32 tensor unless stated:
  a. bine_mx_quant_segments to e4m3 (5 + 1/32 B / element) against
     bine_quant_segments to e4m3 with the scales given (5 B / element) --
     judged: the ratio of times within max(spread, 5 %) of the ratio of bytes;
  b. the same to e2m1 (4.5 + 1/32 B / element), and from bfloat16 -- reported;
  c. one mx_quant_segments against the three per-tensor calls it replaces
     (amax_segments, fp8_scales, quant_segments) -- reported;
  d. bine_mx_dequant_segments against bine_dequant_segments -- reported;
  e. 1,024 tensors x 16 KiB: one call against 1,024 -- reported;
  f. loopback P = 2 and 4 on ONE GPU, 64 Mi elements over the ranks:
     mx_quant_multi against quant_multi and against allgather_multi of the
     bfloat16 copy -- wall clock, reported only: peer memory is local here, so
     this says nothing about xGMI.
a - e: hipEvents around each timed call, 20 timed calls after 5, the C entry
points called with argument arrays built beforehand; f: wall clock around the
loopback driver, 10 timed calls after 2.  Three interleaved rounds each.  The
timers and the rounds are tools/multi_bw.py's.  Random data.  One GPU.
usage: python tools/mx_bw.py > profiles/mx_bw.txt
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, timed, wall  # noqa: E402

FLOAT, BF16 = pico_amd.DTYPES["float"], pico_amd.EXT_DTYPES["bfloat16"]
E4M3, E2M1 = 0, 2


def compare(title, variants, base, timer=timed, want=None):
    """variants: {name: fn}, timed in interleaved rounds; every other variant's
    median of rounds as a ratio of `base`'s; want = {name: the ratio of bytes}:
    judged within max(spread of base, 5 %) of it"""
    print(f"\n{title}", flush=True)
    med = {k: [] for k in variants}
    for rnd in range(ROUNDS):
        for k, fn in variants.items():
            m, lo, hi = timer(fn)
            med[k].append(m)
            print(f"  round {rnd} {k:<44} {m:10.2f} us ({lo:.2f} .. {hi:.2f})", flush=True)
    b = statistics.median(med[base])
    spread = (max(med[base]) - min(med[base])) / b
    print(f"  {base}: median of rounds {b:.2f} us, spread between rounds {100 * spread:.1f} %")
    for k in variants:
        if k == base:
            continue
        m = statistics.median(med[k])
        sk = (max(med[k]) - min(med[k])) / m
        verdict = ""
        if want and k in want:
            tol = max(spread, 0.05)
            ok = m / b <= want[k] * (1 + tol)
            verdict = (f"; bytes ratio {want[k]:.4f}, margin max(spread of base, 5 %) = {100 * tol:.1f} %: "
                       f"{'within' if ok else 'OUTSIDE'}")
        print(f"  {k}: median of rounds {m:.2f} us (spread {100 * sk:.1f} %), ratio to base {m / b:.3f}{verdict}")


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")

    def ptrs(*ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def sizes(*c):
        return (ctypes.c_size_t * len(c))(*c)

    N = 64 << 20
    x = torch.randn(N, device=dev)
    xh = x.to(torch.bfloat16)
    q = torch.empty(N, dtype=torch.uint8, device=dev)
    sb = torch.empty(N // 32, dtype=torch.uint8, device=dev)
    y = torch.empty(N, dtype=torch.float32, device=dev)
    px, pxh, pq, psb, py, cN = ptrs(x), ptrs(xh), ptrs(q), ptrs(sb), ptrs(y), sizes(N)
    amax = torch.zeros(1, dtype=torch.int32, device=dev)
    scales = torch.zeros(2, dtype=torch.float32, device=dev)

    def amax_fn():
        assert L.bine_amax_segments(1, px, cN, FLOAT, amax.data_ptr(), stream) == 0

    def scales_fn():
        assert L.bine_fp8_scales(1, amax.data_ptr(), E4M3, scales.data_ptr(), stream) == 0

    def quant():
        assert L.bine_quant_segments(1, px, pq, cN, FLOAT, E4M3, scales.data_ptr(), stream) == 0

    def mx(src=px, dt=FLOAT, fmt=E4M3):
        assert L.bine_mx_quant_segments(1, src, pq, psb, cN, dt, fmt, stream) == 0

    amax_fn(), scales_fn()
    torch.cuda.synchronize()
    base = "quant_segments e4m3, scales given (5 B)"
    compare("a / b. bine_mx_quant_segments against bine_quant_segments to e4m3 with the scales given, 64 Mi elements",
            {base: quant,
             "mx_quant_segments float -> e4m3 (5.03 B)": mx,
             "mx_quant_segments float -> e2m1 (4.53 B)": lambda: mx(fmt=E2M1),
             "mx_quant_segments bfloat16 -> e4m3 (3.03 B)": lambda: mx(pxh, BF16),
             "mx_quant_segments bfloat16 -> e2m1 (2.53 B)": lambda: mx(pxh, BF16, E2M1)},
            base, want={"mx_quant_segments float -> e4m3 (5.03 B)": (5 + 1 / 32) / 5})

    def three():
        amax_fn(), scales_fn(), quant()

    base = "amax_segments + fp8_scales + quant_segments"
    compare("c. one mx_quant_segments against the three per-tensor calls it replaces", {base: three, "mx_quant_segments e4m3": mx},
            base)

    def deq():
        assert L.bine_dequant_segments(1, pq, py, cN, FLOAT, E4M3, scales.data_ptr() + 4, stream) == 0

    def mxdeq():
        assert L.bine_mx_dequant_segments(1, pq, psb, py, cN, FLOAT, E4M3, stream) == 0

    mx()
    base = "dequant_segments e4m3 (5 B)"
    compare("d. bine_mx_dequant_segments against bine_dequant_segments, e4m3 -> float", {base: deq, "mx_dequant_segments e4m3": mxdeq},
            base)
    del y, xh

    # e: 1,024 tensors of 16 KiB
    ts = [torch.randn(4096, device=dev) for _ in range(1024)]
    qs = [torch.empty(4096, dtype=torch.uint8, device=dev) for _ in range(1024)]
    ss = [torch.empty(128, dtype=torch.uint8, device=dev) for _ in range(1024)]
    pt, pqs, pss, ct = ptrs(*ts), ptrs(*qs), ptrs(*ss), sizes(*([4096] * 1024))
    one = [(ptrs(t), ptrs(u), ptrs(s), sizes(4096)) for t, u, s in zip(ts, qs, ss)]

    def one_call():
        assert L.bine_mx_quant_segments(1024, pt, pqs, pss, ct, FLOAT, E4M3, stream) == 0

    def per_tensor():
        for p, u, s, c in one:
            L.bine_mx_quant_segments(1, p, u, s, c, FLOAT, E4M3, stream)

    base = "1,024 x mx_quant_segments"
    compare("e. 1,024 tensors x 16 KiB: mx_quant_segments once against per tensor", {base: per_tensor, "one call": one_call}, base)
    del ts, qs, ss, q, sb

    # f: the collective, on one GPU
    for P in (2, 4):
        comms = pico_amd.Comm.loopback(P, 0)
        c = N // P
        src = [[x[r * c:(r + 1) * c]] for r in range(P)]
        p8 = [[torch.empty(N, dtype=torch.uint8, device=dev)] for _ in range(P)]
        s8 = [[torch.empty(N // 32, dtype=torch.uint8, device=dev)] for _ in range(P)]
        p16 = [[torch.empty(N, dtype=torch.bfloat16, device=dev)] for _ in range(P)]
        scs = [torch.zeros(2, dtype=torch.float32, device=dev) for _ in range(P)]

        def mxm(fmt="e4m3"):
            rc, st = pico_amd.loopback_mx_quant_multi(comms, "ring", p8, s8, src, fmt, shard_counts=[c])
            assert rc == 0, st

        def fp8():
            rc, st = pico_amd.loopback_quant_multi(comms, "recursivedoubling", "ring", p8, src, "e4m3", scs,
                                                   shard_counts=[c])
            assert rc == 0, st

        def bf16():
            rc, st = pico_amd.loopback_allgather_multi(comms, "ring", None, p16, "bfloat16", shard_counts=[c])
            assert rc == 0, st

        base = "allgather_multi bfloat16"
        compare(f"f. loopback P = {P} on one GPU (peer memory is local: nothing about xGMI), {N >> 20} Mi elements "
                f"(wall clock; reported only)",
                {base: bf16, "quant_multi e4m3": fp8, "mx_quant_multi e4m3": mxm, "mx_quant_multi e2m1": lambda: mxm("e2m1")},
                base, timer=wall)
        for cm in comms:
            cm.destroy()
        del p8, s8, p16


if __name__ == "__main__":
    main()
