"""Host arithmetic of the 16-bit floating element types (test infrastructure).

"float16" (IEEE binary16) and "bfloat16" live on the host as uint16 bit
patterns.  reduce_local() states the semantics of include/bine_amd.h: each
pairwise inout (op) in is the correctly rounded result in the 16-bit format
(nearest even, subnormals kept), MAX / MIN select one operand's bits by
`inout > in ? inout : in` (resp. <).  binary16 goes through numpy.float16;
bfloat16 through a binary32 operation on the widened operands and one
round-to-nearest-even on the bits (exact for + and *: 24 >= 2 * 8 + 2).

patched() makes tests/plan_sim.run replay plans with this arithmetic, the way
tests/test_flat_symbolic.py's symbolic() does for expression trees.
"""
import contextlib

import numpy as np

from oracle import oracle as O

TYPES = ("float16", "bfloat16")
CODES = {"float16": 32, "bfloat16": 33}
BF16_QNAN = 0x7FC0


def to_f32(bits, dtype):
    """the values of uint16 bit patterns, exactly, as float32"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """float32 -> bfloat16 bits, round to nearest even; NaN stays NaN"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(BF16_QNAN), r).astype(np.uint16)


def from_f32(x, dtype):
    """float32 values rounded once (nearest even) to the type's bits"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    return f32_to_bf16(x)


def reduce_local(inp, inout, dtype, op="sum"):
    """inout = inout (op) inp on uint16 bit patterns, in place (the signature
    of oracle.reduce_local)"""
    assert inp.dtype == np.uint16 and inout.dtype == np.uint16 and inp.size == inout.size
    a, b = np.ascontiguousarray(inp), inout.copy()
    with np.errstate(all="ignore"):
        if op in ("sum", "prod"):
            if dtype == "float16":
                x, y = b.view(np.float16), a.view(np.float16)
                r = (x + y if op == "sum" else x * y).view(np.uint16)
            else:
                x, y = to_f32(b, dtype), to_f32(a, dtype)
                r = f32_to_bf16(x + y if op == "sum" else x * y)
        else:
            x, y = to_f32(b, dtype), to_f32(a, dtype)    # exact: comparisons in float32
            r = np.where(x > y if op == "max" else x < y, b, a)
    inout[:] = r


@contextlib.contextmanager
def patched():
    """plan_sim.run(..., dtype="float16" | "bfloat16") with this arithmetic"""
    saved = O.reduce_local
    for t in TYPES:
        O.NP_DTYPES[t] = np.uint16
    O.reduce_local = reduce_local
    try:
        yield
    finally:
        O.reduce_local = saved
        for t in TYPES:
            del O.NP_DTYPES[t]


def tree(leaves, dtype, op, swap=0):
    """level-by-level evaluation of the reduction tree (bine_reduce_tree):
    v[i] = v[i] (op) v[i + w], v[i] the inout side (v[i + w] where bit lvl of
    `swap` is set); every level rounds to the 16-bit type"""
    v = [np.array(x, dtype=np.uint16) for x in leaves]
    w, lvl = 1, 0
    while w < len(v):
        for i in range(0, len(v), 2 * w):
            if (swap >> lvl) & 1:
                t = v[i + w].copy()
                reduce_local(v[i], t, dtype, op)
                v[i] = t
            else:
                reduce_local(v[i + w], v[i], dtype, op)
        w *= 2
        lvl += 1
    return v[0]


# ---- inputs ------------------------------------------------------------------

def random_bits(dtype, n, seed):
    """random finite bit patterns, subnormals included: any 16 bits, with an
    all-ones exponent field (inf / NaN) masked out by clearing its lowest bit"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    field, low = (0x7C00, 0x0400) if dtype == "float16" else (0x7F80, 0x0080)
    return np.where((b & field) == field, b & np.uint16(0xFFFF ^ low), b).astype(np.uint16)


def pico_like(dtype, n, seed):
    """pico_core-like values: uniform in 0..100, rounded to the type"""
    rng = np.random.default_rng(seed)
    return from_f32((rng.random(n) * 100.0).astype(np.float32), dtype)


def near_one(dtype, n, seed):
    """uniform in 0.5..1.5, rounded to the type (products of many stay finite)"""
    rng = np.random.default_rng(seed)
    return from_f32((rng.random(n) + 0.5).astype(np.float32), dtype)


def inputs(dtype, n, P, op="sum", seed=1234):
    """the per-rank inputs of the collective tests: pico-like values under
    SUM (every level's rounding shows), random finite bit patterns under MAX /
    MIN (signs, zeros, subnormals), values near one under PROD"""
    f = {"sum": pico_like, "prod": near_one}.get(op, random_bits)
    return [f(dtype, n, seed + r) for r in range(P)]


def specials(dtype):
    """12 values: +-0, +-inf, one NaN, +-1, two subnormals of opposite sign,
    the largest finite value, 1 + ulp, and a value whose sum with 1 is an
    exact rounding tie (ulp(1) / 2: 1 + it lies halfway between 1 and 1 + ulp)"""
    if dtype == "float16":
        v = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x3C00, 0xBC00, 0x0003, 0x8201, 0x7BFF, 0x3C01, 0x1000]
    else:
        v = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xBF80, 0x0003, 0x8041, 0x7F7F, 0x3F81, 0x3B80]
    return np.array(v, dtype=np.uint16)


def special_grid(dtype):
    """(a, b): the 12 x 12 grid of specials() as two 144-element operands"""
    v = specials(dtype)
    return np.repeat(v, v.size), np.tile(v, v.size)


def is_nan(bits, dtype):
    bits = np.asarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def same(got, exp, dtype):
    """bit-equal wherever exp is not NaN, NaN wherever it is"""
    got, exp = np.asarray(got, dtype=np.uint16), np.asarray(exp, dtype=np.uint16)
    if got.shape != exp.shape:
        return False
    nan = is_nan(exp, dtype)
    return bool(np.array_equal(got[~nan], exp[~nan]) and is_nan(got[nan], dtype).all())
