"""float16 / bfloat16 element types, host side: the C ABI's extension range,
the test helper's arithmetic (tests/h16_util.py) against torch's CPU types,
and the flat plans against the literal ones under that arithmetic."""
import numpy as np
import pytest

import h16_util as H
import plan_sim
import pico_amd
from pico_amd import _lib, api

torch = pytest.importorskip("torch")
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def test_abi_extension_range():
    """codes 32 / 33: 2 bytes, SUM / PROD / MAX / MIN only; every other code
    past MPICH's 17 stays invalid; the Python names resolve"""
    L = pico_amd.lib()
    assert pico_amd.EXT_DTYPES == {"float16": 32, "bfloat16": 33}
    assert len(pico_amd.DTYPES) == 17 and not set(pico_amd.DTYPES) & set(pico_amd.EXT_DTYPES)
    for name, code in pico_amd.EXT_DTYPES.items():
        assert L.bine_dtype_size(code) == 2 == _lib.DTYPE_SIZE[name]
        for op, ov in _lib.OPS.items():
            assert bool(L.bine_op_valid(code, ov)) == (op in ("sum", "prod", "max", "min")), (name, op)
        assert not L.bine_op_valid(code, -1) and not L.bine_op_valid(code, 12)
    for code in (17, 31, 34, 35, 64, -1):
        assert L.bine_dtype_size(code) == 0, code
        assert not any(L.bine_op_valid(code, ov) for ov in _lib.OPS.values()), code
    assert api._dtype(torch.bfloat16) == 33 and api._dtype(torch.float16) == 32
    assert api._dtype("float16") == 32 and api._dtype("bfloat16") == 33
    assert api._dtype(None, torch.zeros(1, dtype=torch.bfloat16)) == 33
    assert api._dtype("float") == 8 and api._dtype(torch.float32) == 8
    # the direct transport's in-launch kernels are not provided for them
    for kind in (1, 2):
        for code in (32, 33):
            assert L.bine_dm_launch_cap(kind, code, 0, 8, 1) == -1


def _torch_op(a, b, dtype, op):
    """b (op) a by torch's CPU arithmetic on the 16-bit type, as bits"""
    ta = torch.from_numpy(a.view(np.int16).copy()).view(TORCH_DT[dtype])
    tb = torch.from_numpy(b.view(np.int16).copy()).view(TORCH_DT[dtype])
    r = tb + ta if op == "sum" else tb * ta
    return r.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_helper_matches_torch_cpu(dtype, op):
    """an independent implementation: torch CPU add / mul on 2^20 random
    finite pairs and on the special-value grid"""
    grid = H.special_grid(dtype)
    for a, b in ((H.random_bits(dtype, 1 << 20, 5), H.random_bits(dtype, 1 << 20, 6)), grid):
        exp = _torch_op(a, b, dtype, op)
        got = b.copy()
        H.reduce_local(a, got, dtype, op)
        assert H.same(got, exp, dtype) and H.same(exp, got, dtype), (dtype, op)


@pytest.mark.parametrize("dtype", H.TYPES)
def test_helper_max_min_select_bits(dtype):
    """MAX / MIN on the grid: the rule `io > in ? io : in` (resp. <) restated
    element by element, bits copied (-0 vs +0 and NaN operands included)"""
    a, b = H.special_grid(dtype)
    va, vb = H.to_f32(a, dtype), H.to_f32(b, dtype)
    for op in ("max", "min"):
        got = b.copy()
        H.reduce_local(a, got, dtype, op)
        for k in range(a.size):
            sel = float(vb[k]) > float(va[k]) if op == "max" else float(vb[k]) < float(va[k])
            assert got[k] == (b[k] if sel else a[k]), (dtype, op, k)


@pytest.mark.parametrize("dtype", H.TYPES)
def test_special_grid_nan_count(dtype):
    """the 12 x 12 grid leaves at least 100 pairs per op to compare bit for
    bit: at most 31 results are NaN (sum 25, prod 31, max / min 12)"""
    a, b = H.special_grid(dtype)
    assert a.size == 144
    for op, nans in (("sum", 25), ("prod", 31), ("max", 12), ("min", 12)):
        r = b.copy()
        H.reduce_local(a, r, dtype, op)
        assert int(H.is_nan(r, dtype).sum()) == nans <= 31, (dtype, op)


PLANS = [("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_permute_remap"), ("reduce", "bine_bdw")]


@pytest.mark.parametrize("coll,algo", PLANS)
@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("dtype", H.TYPES)
def test_flat_plans_give_the_literal_bits(coll, algo, P, dtype):
    """every level of the flat forms' trees rounds to the 16-bit type, so the
    flat plans give the literal plans' bits under this arithmetic"""
    with H.patched():
        for op in ("sum", "prod", "max"):
            rc = [3] * P if coll == "reduce_scatter" else None
            sb = H.inputs(dtype, sum(rc) if rc else 3 * P + 5, P, op)
            literal = plan_sim.run(coll, algo, [x.copy() for x in sb], dtype, op, rcounts=rc)
            flat = plan_sim.run(coll, algo, [x.copy() for x in sb], dtype, op, rcounts=rc, chunk_bytes=16,
                                flat_rs=True, flat_ag=True)
            for r in ([0] if coll == "reduce" else range(P)):
                assert np.array_equal(flat[r], literal[r]), (coll, algo, P, dtype, op, r)
    assert "float16" not in plan_sim.O.NP_DTYPES and plan_sim.O.reduce_local is not H.reduce_local


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("n", [3 * 8 + 5, 1024 * 8 + 3])
def test_gpu_inputs_expose_fp32_accumulation(dtype, n):
    """the P = 8 SUM inputs of the GPU tests tell a tree that keeps fp32
    between its levels (rounding once at the end) from the specified one:
    the two results differ in at least one element"""
    sb = H.inputs(dtype, n, 8, "sum")
    level_rounded = H.tree(sb, dtype, "sum")
    v = [H.to_f32(x, dtype) for x in sb]
    w = 1
    while w < 8:
        for i in range(0, 8, 2 * w):
            v[i] = v[i] + v[i + w]
        w *= 2
    assert not np.array_equal(H.from_f32(v[0], dtype), level_rounded)
    # and with the collective itself
    with H.patched():
        out = plan_sim.run("allreduce", "bine_bdw_remap", [x.copy() for x in sb], dtype, "sum")
    total = np.sum([H.to_f32(x, dtype).astype(np.float64) for x in sb], axis=0).astype(np.float32)
    assert not np.array_equal(out[0], H.from_f32(total, dtype))
