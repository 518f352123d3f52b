#!/usr/bin/env python3
"""Times of the fused AdamW step (k_adamw_segs) beside what it is to be compared
with:
  a. bine_adamw_segments on one 64 Mi-element tensor, bfloat16 g and pout (28 B
     per element: 12 read + 12 written of p, m, v, 2 read of g, 2 written of
     pout), against bine_copy moving the same total bytes (14 B read + 14 B
     written per element) -- the rate and the ratio are reported;
  b. the same call against the unfused sequence the library offered before it:
     bine_clip_segments on g, torch's fused AdamW on (p, m, v) with g widened by
     a cast, and a cast pass of p into the bfloat16 parameters -- judged: the
     fused call not slower than that sequence beyond max(spread, 5 %);
  c. 1,024 tensors x 16 KiB (4,096 elements): one call against 1,024
     per-tensor sequences of b -- reported;
  d. the same 64 Mi-element tensor in the vector body and, with m one element
     off p's phase, in the element body -- reported.
hipEvents around each timed call, the C entry points called with argument arrays
built beforehand.  The timers, the rounds and the report are tools/multi_bw.py's.
Random data; a small lr and a gcoef close to 1 keep it in range over the timed
calls.  One GPU.
usage: python tools/adamw_bw.py > profiles/adamw_bw.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, compare, timed  # noqa: E402

FLOAT, BF16 = pico_amd.DTYPES["float"], pico_amd.EXT_DTYPES["bfloat16"]
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)
PEAK = 8e12


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")
    coef = torch.tensor([1.0 - 2.0 ** -20], dtype=torch.float64, device=dev)
    norm2 = torch.tensor([(1.0 / (1.0 - 2.0 ** -20)) ** 2], dtype=torch.float64, device=dev)

    def vp(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def fused_fn(p, m, v, g, o):
        n, c = len(p), (ctypes.c_size_t * len(p))(*[t.numel() for t in p])
        a = (n, vp(p), vp(m), vp(v), vp(g), vp(o), c, BF16, BF16, *HYPER, 1000, coef.data_ptr(), 1.0, stream)

        def f():
            assert L.bine_adamw_segments(*a) == 0
        return f

    def unfused_fn(p, m, v, g, o):
        """what the caller did before: clip g in place, torch's fused AdamW, one cast per tensor"""
        n, c = len(p), (ctypes.c_size_t * len(p))(*[t.numel() for t in p])
        gp = vp(g)
        for t in p:
            t.requires_grad_(False)
        opt = torch.optim.AdamW(p, lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3], weight_decay=HYPER[4], fused=True)
        for t, mm, vv in zip(p, m, v):   # the optimizer works on the same m and v
            opt.state[t] = {"step": torch.tensor(999.0, device=dev), "exp_avg": mm, "exp_avg_sq": vv}

        def f():
            assert L.bine_clip_segments(n, gp, c, BF16, norm2.data_ptr(), 1.0, 0.0, None, stream) == 0
            for t, gg in zip(p, g):
                t.grad = gg.float()
            opt.step()
            for t, oo in zip(p, o):
                oo.copy_(t)
        return f

    def tensors(n, count, mphase=0):
        mk = lambda s=1.0, ph=0: [(torch.randn(count + 4, device=dev) * s)[ph:ph + count] for _ in range(n)]  # noqa
        p, m, v = mk(), mk(0.1, mphase), [x * x for x in mk(0.1)]
        g = [torch.randn(count, device=dev).bfloat16() for _ in range(n)]
        o = [torch.empty(count, dtype=torch.bfloat16, device=dev) for _ in range(n)]
        return p, m, v, g, o

    # a / b / d: one tensor of 64 Mi elements
    N = 64 << 20
    one = tensors(1, N)
    off = tensors(1, N, mphase=1)
    assert [r[4] for r in pico_amd.plan_adamw(*[[t.data_ptr() for t in x] for x in one], [N], "bfloat16",
                                              "bfloat16")] == [0]
    assert [r[4] for r in pico_amd.plan_adamw(*[[t.data_ptr() for t in x] for x in off], [N], "bfloat16",
                                              "bfloat16")] == [1]
    S = 14 * N
    src = torch.empty(S, dtype=torch.uint8, device=dev)
    dst = torch.empty(S, dtype=torch.uint8, device=dev)

    def copy():
        assert L.bine_copy(dst.data_ptr(), src.data_ptr(), S, stream) == 0

    fused = fused_fn(*one)
    base = "bine_copy of 14 B/element (moves 28)"
    compare(f"a. bine_adamw_segments, one {N >> 20} Mi-element tensor, bfloat16 g and pout (28 B per element), "
            f"against bine_copy of the same bytes", {base: copy, "adamw_segments": fused}, base, S)
    m = timed(fused)[0]
    print(f"  adamw_segments: {m:.2f} us = {28 * N / m / 1e6:.2f} TB/s read + written = "
          f"{100 * 28 * N / m * 1e6 / PEAK:.1f} % of 8 TB/s")
    del src, dst

    base = "clip_segments + torch fused AdamW + cast"
    compare(f"b. the same call against the unfused sequence on the same tensor",
            {base: unfused_fn(*tensors(1, N)), "adamw_segments": fused}, base, 0, margin=True)

    compare("d. the same tensor in the vector body and (m one element off p's phase) in the element body",
            {"vector body": fused, "element body": fused_fn(*off)}, "vector body", 0)
    del one, off, fused
    torch.cuda.empty_cache()

    # c: 1,024 tensors of 16 KiB
    many = tensors(1024, 4096)
    base = "1,024 x (clip + torch fused AdamW + cast)"
    per = tensors(1024, 4096)
    singles = [unfused_fn([per[0][k]], [per[1][k]], [per[2][k]], [per[3][k]], [per[4][k]]) for k in range(1024)]

    def per_tensor():
        for f in singles:
            f()

    compare("c. 1,024 tensors x 16 KiB: one adamw_segments against 1,024 per-tensor sequences",
            {base: per_tensor, "1 x adamw_segments": fused_fn(*many)}, base, 0)


if __name__ == "__main__":
    main()
