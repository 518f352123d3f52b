#!/usr/bin/env python3
"""Times of the MX gradient reduce-scatter's summing kernel and of the call
beside what they are to be compared with:
  a. bine_mx_sum_segments, 8 streams of e4m3 into one 64 Mi-element float32
     tensor (8 * (1 + 1/32) + 4 B / element read and written) against bine_copy
     moving the same total bytes -- judged: the ratio of times within
     max(spread, 5 %) of 1;
  b. e2m1 into bfloat16, 2 and 4 streams (2 * (1/2 + 1/32) + 2 and 4 * ... + 2
     B / element), each against bine_copy of the same total bytes -- reported;
  c. 1,024 tensors of 16 Ki elements: one call against 1,024 -- reported;
  d. loopback P = 2 and 4 on ONE GPU, 64 Mi gradient elements per rank:
     mx_reduce_scatter_multi against reduce_scatter_multi of the float bucket --
     wall clock, reported only: peer memory is local here, so this says nothing
     about xGMI.
a - c: hipEvents around each timed call, 20 timed calls after 5, the C entry
points called with argument arrays built beforehand; d: wall clock around the
loopback driver, 10 timed calls after 2.  Three interleaved rounds each.  The
timers and the rounds are tools/multi_bw.py's, the table tools/mx_bw.py's.
Random bytes, scale bytes around 127.  One GPU.
usage: python tools/mxrs_bw.py > profiles/mxrs_bw.txt
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

    def blocks(counts, fmt, ns):
        """ns wire blocks of random data bytes with scale bytes 120 .. 134"""
        D, B = pico_amd.mx_wire_bytes(counts, fmt)
        t = torch.randint(0, 256, (ns, B), dtype=torch.uint8, device=dev)
        t[:, D:] = torch.randint(120, 135, (ns, B - D), dtype=torch.uint8, device=dev)
        return t, B

    N = 64 << 20
    cN = sizes(N)
    cp_src = torch.empty(N * 49 // 8, dtype=torch.uint8, device=dev)           # 6.125 N bytes: the largest copy below
    cp_dst = torch.empty_like(cp_src)

    def copy_of(total):
        """bine_copy reading and writing `total` bytes in all"""
        return lambda: L.bine_copy(cp_dst.data_ptr(), cp_src.data_ptr(), total // 2, stream)

    for title, fmt, ddt, tdt, cases, judged in (
            ("a. bine_mx_sum_segments, e4m3 -> float, 8 streams, 64 Mi elements, against bine_copy of the same bytes",
             E4M3, FLOAT, torch.float32, (8,), True),
            ("b. bine_mx_sum_segments, e2m1 -> bfloat16, 2 and 4 streams, against bine_copy of the same bytes",
             E2M1, BF16, torch.bfloat16, (2, 4), False)):
        y = torch.empty(N, dtype=tdt, device=dev)
        py = ptrs(y)
        for ns in cases:
            pk, B = blocks([N], fmt, ns)
            total = ns * B + N * y.element_size()

            def mxsum():
                assert L.bine_mx_sum_segments(1, ns, pk.data_ptr(), B, py, cN, ddt, fmt, 1.0, stream) == 0

            base = f"bine_copy, {total / N:.3f} B / element read + written"
            name = f"mx_sum_segments {ns} streams"
            compare(f"{title} ({ns} streams)", {base: copy_of(total), name: mxsum}, base,
                    want={name: 1.0} if judged else None)
            del pk
        del y
    del cp_src, cp_dst

    # c: 1,024 tensors of 16 Ki elements, 4 streams of e4m3 into float
    cnt = [16384] * 1024
    pk, B = blocks(cnt, E4M3, 4)
    D = pico_amd.mx_wire_bytes(cnt, E4M3)[0]
    ts = [torch.empty(16384, device=dev) for _ in cnt]
    pt, ct = ptrs(*ts), sizes(*cnt)
    B1 = pico_amd.mx_wire_bytes([16384], E4M3)[1]
    singles = [torch.randint(100, 140, (4, B1), dtype=torch.uint8, device=dev) for _ in range(8)]   # reused round robin
    one = [(ptrs(t), singles[k % 8].data_ptr()) for k, t in enumerate(ts)]
    c1 = sizes(16384)

    def one_call():
        assert L.bine_mx_sum_segments(1024, 4, pk.data_ptr(), B, pt, ct, FLOAT, E4M3, 1.0, stream) == 0

    def per_tensor():
        for p, s in one:
            L.bine_mx_sum_segments(1, 4, s, B1, p, c1, FLOAT, E4M3, 1.0, stream)

    base = "1,024 x mx_sum_segments"
    compare("c. 1,024 tensors x 16 Ki elements, 4 streams of e4m3 -> float: mx_sum_segments once against per tensor",
            {base: per_tensor, "one call": one_call}, base)
    del ts, pk, singles, D

    # d: the collective, on one GPU
    for P in (2, 4):
        comms = pico_amd.Comm.loopback(P, 0)
        c = N // P
        grads = [[torch.randn(N, device=dev)] for _ in range(P)]
        shards = [[torch.empty(c, device=dev)] for _ in range(P)]
        ws = {f: ([torch.empty(P * pico_amd.mx_wire_bytes([c], f)[1], dtype=torch.uint8, device=dev) for _ in range(P)],
                  [torch.empty(P * pico_amd.mx_wire_bytes([c], f)[1], dtype=torch.uint8, device=dev) for _ in range(P)])
              for f in ("e4m3", "e2m1")}

        def mxrs(fmt="e4m3"):
            rc, st = pico_amd.loopback_mx_reduce_scatter_multi(comms, grads, shards, fmt, shard_counts=[c],
                                                               send_ws=ws[fmt][0], recv_ws=ws[fmt][1])
            assert rc == 0, st

        def rs():
            rc, st = pico_amd.loopback_reduce_scatter_multi(comms, "bine_permute_remap", grads, shards, "float", "sum")
            assert rc == 0, st

        base = "reduce_scatter_multi float"
        compare(f"d. loopback P = {P} on one GPU (peer memory is local: nothing about xGMI), {N >> 20} Mi gradient "
                f"elements per rank (wall clock; reported only)",
                {base: rs, "mx_reduce_scatter_multi e4m3": mxrs, "mx_reduce_scatter_multi e2m1": lambda: mxrs("e2m1")},
                base, timer=wall)
        for cm in comms:
            cm.destroy()
        del grads, shards, ws


if __name__ == "__main__":
    main()
