#!/usr/bin/env python3
"""Times of the FP8 quantization kernels beside what they are to be compared
with, one 64 Mi-element float32 tensor unless stated:
  a. bine_quant_segments to e4m3 (5 B / element) against bine_narrow to bfloat16
     of the same tensor (6 B / element) -- judged: not slower than the narrow
     beyond max(spread, 5 %);
  b. bine_amax_segments against bine_sumsq_segments on the same tensor (the same
     bytes read) -- judged by the same rule;
  c. loopback P = 2 and 4 on ONE GPU, 64 Mi elements over the ranks: quant_multi
     to e4m3 against allgather_multi of the bfloat16 copy -- wall clock,
     reported only: peer memory is local here, so this says nothing about xGMI;
  d. 1,024 tensors x 16 KiB: one amax + scales + quant call each against 1,024
     per-tensor sequences -- reported only.
a, b, d: hipEvents around each timed call, 20 timed calls after 5, the C entry
points called with argument arrays built beforehand; c: wall clock around the
loopback driver, which synchronizes every rank before it returns, 10 timed
calls after 2.  Three interleaved rounds each.  The timers, the rounds and the
report are tools/multi_bw.py's.  Random data.  One GPU.
usage: python tools/fp8_bw.py > profiles/fp8_bw.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, compare, wall  # noqa: E402

FLOAT, BF16 = pico_amd.DTYPES["float"], pico_amd.EXT_DTYPES["bfloat16"]
E4M3 = 0


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")

    def lists(ts):
        n = len(ts)
        return n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]), (ctypes.c_size_t * n)(*[t.numel() for t in ts])

    N = 64 << 20
    x = torch.randn(N, device=dev)
    q = torch.empty(N, dtype=torch.uint8, device=dev)
    h = torch.empty(N, dtype=torch.bfloat16, device=dev)
    n1, px, cx = lists([x])
    pq = (ctypes.c_void_p * 1)(q.data_ptr())
    amax = torch.zeros(1, dtype=torch.int32, device=dev)
    scales = torch.zeros(2, dtype=torch.float32, device=dev)
    assert L.bine_amax_segments(1, px, cx, FLOAT, amax.data_ptr(), stream) == 0
    assert L.bine_fp8_scales(1, amax.data_ptr(), E4M3, scales.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    print(f"\namax of {N >> 20} Mi float32: {float(amax.view(torch.float32)[0])!r} (torch {float(x.abs().max())!r}), "
          f"scale {float(scales[0])!r}")

    def quant():
        assert L.bine_quant_segments(1, px, pq, cx, FLOAT, E4M3, scales.data_ptr(), stream) == 0

    def narrow():
        assert L.bine_narrow(x.data_ptr(), h.data_ptr(), N, BF16, stream) == 0

    base = "bine_narrow to bfloat16 (6 B/elt)"
    compare("a. bine_quant_segments to e4m3 (5 B / element) against bine_narrow to bfloat16 (6 B / element)",
            {base: narrow, "quant_segments e4m3": quant}, base, 0, margin=True)

    need = pico_amd.plan_sumsq([x.data_ptr()], [N], "float")
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    scratch = torch.zeros(max(need, 1), dtype=torch.float64, device=dev)

    def sumsq():
        assert L.bine_sumsq_segments(1, px, cx, FLOAT, out.data_ptr(), scratch.data_ptr(), need, stream) == 0

    def amax_fn():
        assert L.bine_amax_segments(1, px, cx, FLOAT, amax.data_ptr(), stream) == 0

    base = "bine_sumsq_segments"
    compare("b. bine_amax_segments against bine_sumsq_segments on the same 256 MiB (the same bytes read)",
            {base: sumsq, "amax_segments": amax_fn}, base, 0, margin=True)
    del h, q

    # d: 1,024 tensors of 16 KiB
    ts = [torch.randn(4096, device=dev) for _ in range(1024)]
    qs = [torch.empty(4096, dtype=torch.uint8, device=dev) for _ in range(1024)]
    n, pt, ct = lists(ts)
    pqs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in qs])
    am = torch.zeros(n, dtype=torch.int32, device=dev)
    sc = torch.zeros(2 * n, dtype=torch.float32, device=dev)

    def one_call_each():
        assert L.bine_amax_segments(n, pt, ct, FLOAT, am.data_ptr(), stream) == 0
        assert L.bine_fp8_scales(n, am.data_ptr(), E4M3, sc.data_ptr(), stream) == 0
        assert L.bine_quant_segments(n, pt, pqs, ct, FLOAT, E4M3, sc.data_ptr(), stream) == 0

    one = [lists([t]) + ((ctypes.c_void_p * 1)(u.data_ptr()),) for t, u in zip(ts, qs)]

    def per_tensor():
        for k, (_, p, c, pu) in enumerate(one):
            L.bine_amax_segments(1, p, c, FLOAT, am.data_ptr() + 4 * k, stream)
            L.bine_fp8_scales(1, am.data_ptr() + 4 * k, E4M3, sc.data_ptr() + 8 * k, stream)
            L.bine_quant_segments(1, p, pu, c, FLOAT, E4M3, sc.data_ptr() + 8 * k, stream)

    base = "1,024 x (amax + scales + quant)"
    compare("d. 1,024 tensors x 16 KiB: amax_segments + fp8_scales + quant_segments once against per tensor",
            {base: per_tensor, "one call each": one_call_each}, base, 0)
    del ts, qs

    # c: the collective, on one GPU
    for P in (2, 4):
        comms = pico_amd.Comm.loopback(P, 0)
        c = N // P
        src = [[x[r * c:(r + 1) * c]] for r in range(P)]
        p8 = [[torch.empty(N, dtype=torch.uint8, device=dev)] for _ in range(P)]
        p16 = [[torch.empty(N, dtype=torch.bfloat16, device=dev)] for _ in range(P)]
        scs = [torch.zeros(2, dtype=torch.float32, device=dev) for _ in range(P)]

        def fp8():
            rc, st = pico_amd.loopback_quant_multi(comms, "recursivedoubling", "ring", p8, src, "e4m3", scs,
                                                   shard_counts=[c])
            assert rc == 0, st

        def bf16():
            rc, st = pico_amd.loopback_allgather_multi(comms, "ring", None, p16, "bfloat16", shard_counts=[c])
            assert rc == 0, st

        base = "allgather_multi bfloat16"
        compare(f"c. loopback P = {P} on one GPU (peer memory is local: nothing about xGMI), {N >> 20} Mi elements: "
                f"quant_multi to e4m3 against allgather_multi of the bfloat16 copy (wall clock; reported only)",
                {base: bf16, "quant_multi e4m3": fp8}, base, 0, timer=wall)
        for cm in comms:
            cm.destroy()
        del p8, p16


if __name__ == "__main__":
    main()
