#!/usr/bin/env python3
"""Times of MX quantization with an error-feedback residual beside what they are
to be compared with:
  a. bine_mx_quant_ef_segments, float -> e4m3, 64 Mi elements (4 + 4 read, 4 + 1
     + 1/32 written: 13 + 1/32 B / element) against bine_copy moving the same
     total bytes -- judged: the ratio of times within max(spread, 5 %) of 1;
  b. the same call against bine_mx_quant_segments on the same source (5 + 1/32
     B / element): the traffic ratio predicts 2.59 -- reported;
  c. bfloat16 -> e2m1 (2 + 4 read, 4 + 1/2 + 1/32 written: 10.5 + 1/32 B /
     element) against bine_copy of the same total bytes -- reported;
  d. 1,024 tensors of 16 Ki elements: one call against 1,024 -- reported;
  e. loopback P = 2 and 4 on ONE GPU, 64 Mi gradient elements per rank:
     mx_reduce_scatter_multi_ef against mx_reduce_scatter_multi -- wall clock,
     reported only: peer memory is local here, so this says nothing about xGMI.
a - d: hipEvents around each timed call, 20 timed calls after 5, the C entry
points called with argument arrays built beforehand; e: wall clock around the
loopback driver, 10 timed calls after 2.  Three interleaved rounds each.  The
timers and the rounds are tools/multi_bw.py's, the table tools/mx_bw.py's.
Normal gradients; the residual is carried from call to call, as in use.  One GPU.
usage: python tools/mxef_bw.py > profiles/mxef_bw.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, wall  # noqa: E402
from mx_bw import compare  # noqa: E402

FLOAT, BF16 = pico_amd.DTYPES["float"], pico_amd.EXT_DTYPES["bfloat16"]
E4M3, E2M1 = 0, 2


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
    cN = sizes(N)
    cp_src = torch.empty(N * 417 // 64, dtype=torch.uint8, device=dev)         # (13 + 1/32) / 2 N bytes: the largest copy
    cp_dst = torch.empty_like(cp_src)
    res = torch.zeros(N, device=dev)
    sc = torch.empty(N // 32, dtype=torch.uint8, device=dev)
    pr, ps = ptrs(res), ptrs(sc)

    for title, fmt, sdt, tdt, per, plain in (
            ("a, b. bine_mx_quant_ef_segments, float -> e4m3, 64 Mi elements, against bine_copy of the same bytes and "
             "against bine_mx_quant_segments", E4M3, FLOAT, torch.float32, 13 + 1 / 32, True),
            ("c. bine_mx_quant_ef_segments, bfloat16 -> e2m1, 64 Mi elements, against bine_copy of the same bytes",
             E2M1, BF16, torch.bfloat16, 10.5 + 1 / 32, False)):
        x = torch.randn(N, device=dev).to(tdt)
        d8 = torch.empty(pico_amd.mx_dbytes(N, fmt), dtype=torch.uint8, device=dev)
        px, pd = ptrs(x), ptrs(d8)
        total = int(per * N)
        res.zero_()

        def ef():
            assert L.bine_mx_quant_ef_segments(1, px, pr, pd, ps, cN, sdt, fmt, stream) == 0

        def mxq():
            assert L.bine_mx_quant_segments(1, px, pd, ps, cN, sdt, fmt, stream) == 0

        def copy():
            L.bine_copy(cp_dst.data_ptr(), cp_src.data_ptr(), total // 2, stream)

        base = f"bine_copy, {per:.3f} B / element read + written"
        variants = {base: copy, "mx_quant_ef_segments": ef}
        if plain:
            variants["mx_quant_segments (5.031 B / element)"] = mxq
        compare(title, variants, base, want={"mx_quant_ef_segments": 1.0} if plain else None)
        del x, d8
    del cp_src, cp_dst, res, sc

    # d: 1,024 tensors of 16 Ki elements, float -> e4m3
    cnt = [16384] * 1024
    xs = [torch.randn(16384, device=dev) for _ in cnt]
    rs = [torch.zeros(16384, device=dev) for _ in cnt]
    ds = [torch.empty(16384, dtype=torch.uint8, device=dev) for _ in cnt]
    ss = [torch.empty(512, dtype=torch.uint8, device=dev) for _ in cnt]
    px, pr, pd, ps, ct = ptrs(*xs), ptrs(*rs), ptrs(*ds), ptrs(*ss), sizes(*cnt)
    one = [(ptrs(a), ptrs(b), ptrs(c), ptrs(d)) for a, b, c, d in zip(xs, rs, ds, ss)]
    c1 = sizes(16384)

    def one_call():
        assert L.bine_mx_quant_ef_segments(1024, px, pr, pd, ps, ct, FLOAT, E4M3, stream) == 0

    def per_tensor():
        for a, b, c, d in one:
            L.bine_mx_quant_ef_segments(1, a, b, c, d, c1, FLOAT, E4M3, stream)

    base = "1,024 x mx_quant_ef_segments"
    compare("d. 1,024 tensors x 16 Ki elements, float -> e4m3: mx_quant_ef_segments once against per tensor",
            {base: per_tensor, "one call": one_call}, base)
    del xs, rs, ds, ss

    # e: the collective, on one GPU
    for P in (2, 4):
        comms = pico_amd.Comm.loopback(P, 0)
        c = N // P
        grads = [[torch.randn(N, device=dev)] for _ in range(P)]
        resid = [[torch.zeros(N, device=dev)] for _ in range(P)]
        shards = [[torch.empty(c, device=dev)] for _ in range(P)]
        ws = {f: ([torch.empty(P * pico_amd.mx_wire_bytes([c], f)[1], dtype=torch.uint8, device=dev) for _ in range(P)],
                  [torch.empty(P * pico_amd.mx_wire_bytes([c], f)[1], dtype=torch.uint8, device=dev) for _ in range(P)])
              for f in ("e4m3", "e2m1")}

        def mxrs(fmt="e4m3"):
            rc, st = pico_amd.loopback_mx_reduce_scatter_multi(comms, grads, shards, fmt, shard_counts=[c],
                                                               send_ws=ws[fmt][0], recv_ws=ws[fmt][1])
            assert rc == 0, st

        def mxef(fmt="e4m3"):
            rc, st = pico_amd.loopback_mx_reduce_scatter_multi_ef(comms, grads, resid, shards, fmt, shard_counts=[c],
                                                                  send_ws=ws[fmt][0], recv_ws=ws[fmt][1])
            assert rc == 0, st

        base = "mx_reduce_scatter_multi e4m3"
        compare(f"e. loopback P = {P} on one GPU (peer memory is local: nothing about xGMI), {N >> 20} Mi gradient "
                f"elements per rank (wall clock; reported only)",
                {base: mxrs, "mx_reduce_scatter_multi_ef e4m3": mxef,
                 "mx_reduce_scatter_multi e2m1": lambda: mxrs("e2m1"),
                 "mx_reduce_scatter_multi_ef e2m1": lambda: mxef("e2m1")}, base, timer=wall)
        for cm in comms:
            cm.destroy()
        del grads, resid, shards, ws


if __name__ == "__main__":
    main()
