#!/usr/bin/env python3
"""Times of the dynamic (loss-scaled, skipping) AdamW step beside the plain one:
  a. bine_adamw_segments_dyn (skip = 0) against bine_adamw_segments on one 64
     Mi-element tensor, bfloat16 g and pout (28 B per element): the same memory
     traffic plus one 96-byte read of the state per workgroup -- judged: the
     dynamic form not slower beyond max(spread, 5 %);
  b. the same call with skip = 1 (every workgroup issues its tile's loads,
     reads the state and returns before its first store) -- reported;
  c. bine_step_update alone (one thread) -- reported.
hipEvents around each timed call, the C entry points called with argument arrays
built beforehand.  The timers, the rounds and the report are tools/multi_bw.py's.
Random data; both forms run step 1,000 at the same hyper-parameters with a
multiplier of (nearly) 1, a small lr keeps the values in range over the timed
calls.  One GPU.
usage: python tools/step_bw.py > profiles/step_bw.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pico_amd  # noqa: E402
from multi_bw import ITERS, ROUNDS, WARM, compare  # noqa: E402
from pico_amd import _lib  # noqa: E402

BF16 = pico_amd.EXT_DTYPES["bfloat16"]
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def main():
    dev = torch.device("cuda:0")
    L = pico_amd.lib()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"device: {torch.cuda.get_device_name(0)}; {ITERS} timed calls after {WARM} warm-up, {ROUNDS} rounds per "
          f"variant (interleaved); us = median of a round (min .. max)")
    coef = torch.tensor([1.0 - 2.0 ** -20], dtype=torch.float64, device=dev)

    def state(norm2):
        """step 999 + one update on the host: step 1,000; growth far away, so the scale stays 1"""
        st = pico_amd.step_state_init(1.0, 999, HYPER["beta1"], HYPER["beta2"])
        pico_amd.step_update_host(st, norm2, growth_interval=10 ** 9, **HYPER)
        return torch.from_numpy(st.copy()).to(dev)

    taken, skipped = state(1.0), state(float("inf"))
    assert pico_amd.step_state_read(taken)["skip"] == 0.0 and pico_amd.step_state_read(taken)["gm"] == 1.0
    assert pico_amd.step_state_read(skipped)["skip"] == 1.0

    N = 64 << 20
    mk = lambda s=1.0: (torch.randn(N, device=dev) * s)  # noqa: E731
    p, m, v = mk(), mk(0.1), mk(0.1) ** 2
    g = torch.randn(N, device=dev).bfloat16()
    o = torch.empty(N, dtype=torch.bfloat16, device=dev)
    vp = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    c = (ctypes.c_size_t * 1)(N)
    lists = (1, vp(p), vp(m), vp(v), vp(g), vp(o), c, BF16, BF16)
    assert [r[4] for r in pico_amd.plan_adamw(*[[t.data_ptr()] for t in (p, m, v, g, o)], [N], "bfloat16",
                                              "bfloat16")] == [0]
    plain_args = lists + (*HYPER.values(), 1000, coef.data_ptr(), 1.0, stream)

    def plain():
        assert L.bine_adamw_segments(*plain_args) == 0

    def dyn(st):
        a = lists + (st.data_ptr(), stream)

        def f():
            assert L.bine_adamw_segments_dyn(*a) == 0
        return f

    base = "adamw_segments"
    compare(f"a. bine_adamw_segments_dyn (skip = 0) against bine_adamw_segments, one {N >> 20} Mi-element tensor, "
            f"bfloat16 g and pout (28 B per element)", {base: plain, "adamw_segments_dyn": dyn(taken)}, base, 0,
            margin=True)
    compare("b. the same tensor, skip = 1: loads issued, nothing stored",
            {base: plain, "adamw_segments_dyn, skipped": dyn(skipped)}, base, 0)

    norm2 = torch.tensor([3.0], dtype=torch.float64, device=dev)
    scratch = state(1.0)
    h = _lib.StepHyper(*HYPER.values(), float("inf"), 1e-6, 2.0, 0.5, 1.0, 2.0 ** 24, 2000)
    upd = (scratch.data_ptr(), norm2.data_ptr(), ctypes.byref(h), stream)

    def update():
        assert L.bine_step_update(*upd) == 0

    dst = torch.zeros(1, dtype=torch.float64, device=dev)

    def empty_copy():
        assert L.bine_copy(dst.data_ptr(), norm2.data_ptr(), 8, stream) == 0

    base = "bine_copy of 8 bytes (a launch)"
    compare("c. bine_step_update alone, beside the smallest launch the library has",
            {base: empty_copy, "step_update": update}, base, 0)


if __name__ == "__main__":
    main()
