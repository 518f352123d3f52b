"""Host statement of the wide (binary32-accumulating) reductions (test
infrastructure): include/bine_amd.h's definition, computed without the code
under test.

A wide call returns narrow(F): the inputs (uint16 bit patterns,
tests/h16_util.py) are widened exactly to float32 (h16_util.to_f32), F is the
BINE_FLOAT call's result on them -- the host replay of the float plan
(tests/plan_sim.py, the oracle's MPI_Reduce_local) for the collectives, the
oracle's reduce_local level by level for a tree -- times float32(scale) in
float32 when scale != 1.0 (scale_sim.S), and narrow is ONE round-to-nearest-
even into the 16-bit format (h16_util.from_f32).
"""
import numpy as np

import h16_util as H
import plan_sim
import scale_sim as SS
from oracle import oracle as O


def narrow(f, dtype, scale=1.0):
    f = np.ascontiguousarray(f, dtype=np.float32)
    if scale != 1.0:
        f = SS.S(f, "float", scale)
    return H.from_f32(f, dtype)


def collective(coll, algo, sbufs, dtype, op="sum", rcounts=None, in_place=False, scale=1.0):
    """every rank's expected output bits; raises pico_amd.BineError where the
    float call's plan fails (the wide call then returns that status)"""
    x = [H.to_f32(b, dtype) for b in sbufs]
    f = plan_sim.run(coll, algo, x, "float", op, rcounts=rcounts, in_place=in_place)
    return [narrow(y, dtype, scale) for y in f]


def tree(leaves, dtype, op="sum", swap=0, scale=1.0):
    """bine_reduce_tree_wide: v[i] = v[i] (op) v[i + w] level by level in
    float32, v[i] the inout side (v[i + w] where bit lvl of `swap` is set)"""
    v = [H.to_f32(x, dtype).copy() for x in leaves]
    w, lvl = 1, 0
    with np.errstate(all="ignore"):
        while w < len(v):
            for i in range(0, len(v), 2 * w):
                if (swap >> lvl) & 1:
                    t = v[i + w].copy()
                    O.reduce_local(np.ascontiguousarray(v[i]), t, "float", op)
                    v[i] = t
                else:
                    O.reduce_local(np.ascontiguousarray(v[i + w]), v[i], "float", op)
            w *= 2
            lvl += 1
        return narrow(v[0], dtype, scale)
