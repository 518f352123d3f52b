#!/usr/bin/env python3
"""k_reduce's capped grid in the two compilations of pico_amd/csrc/kernels.hip
that bine_set_reduce_tuning does not reach: the float16 / bfloat16 kernels and
the logical / bitwise / MAXLOC / MINLOC ones (with the pair and the complex
types).  Both read BINE_REDUCE_MAXBLOCKS once, at their first call, so the
multi-trip path is reachable only from a process started with it set.  Run as

    BINE_REDUCE_MAXBLOCKS=2 BINE_REDUCE_UNROLL=8 python tools/reduce_env_check.py

(tests/test_gpu_reduce_variants.py does, in a child process).  Every (type, op)
runs the two multi-trip shapes of tests/reduce_variants_cases.py for the
kernel's U (second trips, a workgroup split across the loop boundary; a
partial tile after full trips that holds the last vector:
tests/test_reduce_variants_cases.py) at both phases, in
place and out of place, inside an arena of guard bytes, bit for bit against
tests/h16_util.py or the oracle:

  float16, bfloat16 x sum, prod, max, min
  the eight integer types x land, band, lor, bor, lxor, bxor
  float, double x land, lor, lxor
  the five pair types x maxloc, minloc
  the two complex types x sum, prod
  float x sum (the first compilation, which reads BINE_REDUCE_* itself as long
  as bine_set_reduce_tuning was not called: U = 8 with the table's U = 8 shape)

Values only: the process cannot see how many workgroups a launch had.  Prints
one RESULT line; exits non-zero on any mismatch, after naming the type, op,
phase, form and first differing byte."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import h16_util as H  # noqa: E402
import reduce_variants_cases as C  # noqa: E402
from oracle import oracle as O  # noqa: E402

INTS = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64")
WANT_ENV = {"BINE_REDUCE_MAXBLOCKS": "2", "BINE_REDUCE_UNROLL": "8"}


def pairs():
    """(dtype, op, U of the kernel that runs it)"""
    out = [(t, op, C.DEFAULT_U) for t in H.TYPES for op in ("sum", "prod", "max", "min")]
    out += [(t, op, C.DEFAULT_U) for t in INTS for op in ("land", "band", "lor", "bor", "lxor", "bxor")]
    out += [(t, op, C.DEFAULT_U) for t in ("float", "double") for op in ("land", "lor", "lxor")]
    out += [(t, op, C.DEFAULT_U) for t in O.PAIRS for op in ("maxloc", "minloc")]
    out += [(t, op, C.DEFAULT_U) for t in ("c_float_complex", "c_double_complex") for op in ("sum", "prod")]
    return out + [("float", "sum", int(WANT_ENV["BINE_REDUCE_UNROLL"]))]


def np_of(dtype):
    return np.dtype(np.uint16 if dtype in H.TYPES else O.NP_DTYPES[dtype])


def operands(dtype, op, n):
    if dtype in H.TYPES:
        return H.inputs(dtype, n, 2, op, seed=900)
    return [O.sparsify(O.fill(dtype, n, 900 + j), dtype, j) for j in range(2)]


def h16_same(dtype):
    def same(got, want):
        return H.same(np.frombuffer(got.tobytes(), np.uint16), np.frombuffer(want.tobytes(), np.uint16), dtype)
    return same


def main():
    t0 = time.time()
    for k, v in WANT_ENV.items():
        if os.environ.get(k) != v:
            print(f"RESULT not run: {k} must be {v} in the environment")
            return 2
    import torch

    import pico_amd
    assert torch.cuda.is_available(), "needs an MI355X"
    runs = bad = 0
    for dtype, op, U in pairs():
        nd = np_of(dtype)
        for nvec, phase in [(nv, ph) for nv in (C.multi(U), C.partial(U)) for ph in C.PHASES]:
            assert C.blocks_of(nvec, U, int(WANT_ENV["BINE_REDUCE_MAXBLOCKS"])) == 2
            n = C.elements(nvec, nd.itemsize, phase)
            a, b = operands(dtype, op, n)
            exp = b.copy()
            (H.reduce_local if dtype in H.TYPES else O.reduce_local)(a, exp, dtype, op)
            ar = C.Arena(a, b, (phase,) * 3)
            ar.upload()
            for inplace in (False, True):
                ar.reset()
                if inplace:
                    pico_amd.reduce_local(ar.ptr(0), ar.ptr(1), n, dtype, op)
                else:
                    pico_amd.reduce3(ar.ptr(0), ar.ptr(1), ar.ptr(2), n, dtype, op)
                torch.cuda.synchronize()
                diff = ar.first_difference(ar.expected(exp, inplace),
                                           ignore=C.padding_mask(ar, nd, 1 if inplace else 2),
                                           same=h16_same(dtype) if dtype in H.TYPES else None)
                runs += 1
                if diff is not None:
                    bad += 1
                    print(f"MISMATCH {dtype} {op} phase={phase} {'in place' if inplace else 'out of place'} "
                          f"n={n}: {diff}", flush=True)
    print(f"RESULT runs={runs} bad={bad} wall={time.time() - t0:.1f}s", flush=True)
    return 0 if runs == 8 * len(pairs()) and bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
