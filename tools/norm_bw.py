#!/usr/bin/env python3
"""Times of the segmented sum of squares (k_sumsq_segs) and the segmented scale
(k_scale_segs) beside what they are to be compared with:
  1. bine_sumsq_segments on one 256 MiB float tensor (reads S bytes), with plain
     and with non-temporal loads (BINE_SUMSQ_NT), against bine_copy of the same
     256 MiB (moves 2 S) -- judged: not slower than the copy beyond max(spread,
     5 %); the fraction of 8 TB/s is printed;
  2. bine_clip_segments with c < 1 on one 256 MiB float tensor against in-place
     bine_scale on the same bytes -- judged by the same rule;
  3. 1,024 tensors x 16 KiB: one sumsq_segments + one clip_segments against
     1,024 bine_scale calls plus 1,024 per-tensor torch norms -- the ratio is
     reported;
  4. loopback P = 4, 64 float tensors of 64 Ki elements per rank: one
     clip_multi (bine_lat) against sumsq_segments + loopback_allreduce +
     clip_segments per rank -- wall clock, reported only (the loopback
     driver's host cost bounds both sides).
1 - 3: hipEvents around each timed call, the C entry points called with
argument arrays built beforehand; 4: wall clock.  The timers, the rounds and the
report are tools/multi_bw.py's.  Random data.  One GPU.
usage: python tools/norm_bw.py > profiles/norm_bw.txt
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

FLOAT = pico_amd.DTYPES["float"]
PEAK = 8e12


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")

    def lists(ts):
        n = len(ts)
        return n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]), (ctypes.c_size_t * n)(*[t.numel() for t in ts])

    def sumsq_fn(ts, nt=None):
        n, p, c = lists(ts)
        need = pico_amd.plan_sumsq([t.data_ptr() for t in ts], [t.numel() for t in ts], "float")
        out = torch.zeros(n + 1, dtype=torch.float64, device=dev)
        scratch = torch.zeros(max(need, 1), dtype=torch.float64, device=dev)

        def f():
            if nt is not None:
                os.environ["BINE_SUMSQ_NT"] = nt
            assert L.bine_sumsq_segments(n, p, c, FLOAT, out.data_ptr(), scratch.data_ptr(), need, stream) == 0
        return f, out

    def clip_fn(ts, norm2, max_norm):
        n, p, c = lists(ts)

        def f():
            assert L.bine_clip_segments(n, p, c, FLOAT, norm2.data_ptr(), max_norm, 0.0, None, stream) == 0
        return f

    # 1 / 2: one 256 MiB tensor
    S = 256 << 20
    x = torch.randn(S // 4, device=dev)
    y = torch.empty_like(x)
    plain, out = sumsq_fn([x], "0")
    nontemporal, _ = sumsq_fn([x], "1")
    plain()
    torch.cuda.synchronize()
    ref = float((x.double() ** 2).sum())
    print(f"\nsum of squares of {S >> 20} MiB: {float(out[0]):.17g}, torch float64 {ref:.17g}, relative difference "
          f"{abs(float(out[0]) - ref) / ref:.2e}")

    def copy():
        assert L.bine_copy(y.data_ptr(), x.data_ptr(), S, stream) == 0

    base = "bine_copy 256 MiB (moves 2 S)"
    compare("1. bine_sumsq_segments, one 256 MiB float tensor (reads S), against bine_copy of the same bytes",
            {base: copy, "sumsq, plain loads": plain, "sumsq, non-temporal loads": nontemporal}, base, S, margin=True)
    for name, fn in (("plain", plain), ("non-temporal", nontemporal)):
        from multi_bw import timed
        m = timed(fn)[0]
        print(f"  sumsq {name}: {m:.2f} us = {S / m / 1e6:.2f} TB/s read = {100 * S / m * 1e6 / PEAK:.1f} % of 8 TB/s")
    os.environ.pop("BINE_SUMSQ_NT", None)

    c = 1.0 - 2.0 ** -20      # c < 1, close enough to one that the data keeps its range over the timed calls
    norm2 = torch.tensor([(1.0 / c) ** 2], dtype=torch.float64, device=dev)

    def scale():
        assert L.bine_scale(x.data_ptr(), x.data_ptr(), S // 4, FLOAT, c, stream) == 0

    base = "bine_scale in place 256 MiB"
    compare("2. bine_clip_segments (c < 1), one 256 MiB float tensor, against in-place bine_scale on the same bytes",
            {base: scale, "clip_segments": clip_fn([x], norm2, 1.0)}, base, S, margin=True)
    del y

    # 3: 1,024 tensors of 16 KiB
    ts = [torch.randn(4096, device=dev) for _ in range(1024)]
    one_sumsq, out = sumsq_fn(ts)
    one_clip = clip_fn(ts, out[1024:], 1e30)

    def fused():
        one_sumsq()
        one_clip()

    def per_tensor():
        for t in ts:
            torch.linalg.vector_norm(t)
        for t in ts:
            L.bine_scale(t.data_ptr(), t.data_ptr(), 4096, FLOAT, c, stream)

    base = "1,024 torch norms + 1,024 bine_scale"
    compare("3. 1,024 tensors x 16 KiB: one sumsq_segments + one clip_segments against the per-tensor calls",
            {base: per_tensor, "sumsq_segments + clip_segments": fused}, base, 0)
    del ts

    # 4: the collective
    P, NT = 4, 64
    comms = pico_amd.Comm.loopback(P, 0)
    bufs = [[torch.randn(64 << 10, device=dev) for _ in range(NT)] for _ in range(P)]
    stats = [torch.zeros(NT + 2, dtype=torch.float64, device=dev) for _ in range(P)]

    def one():
        rc, st = pico_amd.loopback_clip_multi(comms, "bine_lat", bufs, "float", 1e30, 1e-6, stats)
        assert rc == 0, st

    def composed():
        vs = [pico_amd.sumsq_segments(bufs[r], "float") for r in range(P)]
        rc, st = pico_amd.loopback_allreduce(comms, "bine_lat", [pico_amd.IN_PLACE] * P, vs, NT + 1, "double", "sum")
        assert rc == 0, st
        for r in range(P):
            pico_amd.clip_segments(bufs[r], vs[r][NT:], 1e30, 1e-6, dtype="float")
        torch.cuda.synchronize()

    base = "sumsq_segments + loopback_allreduce + clip_segments"
    compare(f"4. loopback P = {P}, {NT} float tensors x 64 Ki elements per rank, bine_lat (wall clock; reported only)",
            {base: composed, "1 x clip_multi": one}, base, 0, timer=wall)
    for cm in comms:
        cm.destroy()


if __name__ == "__main__":
    main()
