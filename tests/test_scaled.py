"""Scaled (averaging) allreduce / reduce-scatter, host side: the new ABI, the
scaled schedules against the unscaled ones (identical but for the SCALED flag
and the SCALE primitive), every output element scaled exactly once (host
replay of all ranks, tests/scale_sim.py), where the scale is fused and where
it trails, and that the GPU tests' inputs can tell the specified arithmetic
from the two plausible wrong ones."""
import collections
import ctypes

import numpy as np
import pytest

import h16_util as H
import scale_sim as SS
import pico_amd
from pico_amd import _lib

AR = sorted(pico_amd.ALGOS["allreduce"])
RS = sorted(pico_amd.ALGOS["reduce_scatter"])
PS = [1, 2, 3, 4, 6, 8, 16]
FORMS = {"literal": {}, "flat_rs": {"flat_rs": True}, "flat_rs_ag1": {"flat_rs": True, "flat_ag": True},
         "flat_rs_ag2": {"flat_rs": True, "flat_ag": 2}}
NEW = ["bine_scale_valid", "bine_scale", "bine_reduce_tree_scaled", "bine_allreduce_scaled",
       "bine_reduce_scatter_scaled", "bine_loopback_run_allreduce_scaled", "bine_loopback_run_reduce_scatter_scaled"]


def rcounts_of(algo, P, per):
    """ragged counts (equal ones for permute_remap, which defines no others)"""
    return [per] * P if algo == "bine_permute_remap" else [per + (i % 3) for i in range(P)]


def plans_ok(coll, algo, P, **kw):
    try:
        for r in range(P):
            pico_amd.schedule(coll, algo, P, r, **kw)
        return True
    except pico_amd.BineError:
        return False


# ---- 1. ABI -----------------------------------------------------------------------

def test_abi():
    """the new symbols are exported; bine_scale_valid is 1 exactly on the four
    floating types x sum / prod / max / min; the arithmetic entry points refuse
    every other pair before they touch the GPU (null pointers, no device needed)"""
    sym = _lib.exported_symbols(_lib.CORE)
    assert not [s for s in NEW if s not in sym]
    L = pico_amd.lib()
    good = {(d, o) for d in (8, 9, 32, 33) for o in (0, 1, 2, 3)}
    for d in list(range(-1, 40)):
        for o in range(-1, 14):
            assert L.bine_scale_valid(d, o) == ((d, o) in good), (d, o)
    assert pico_amd.scale_valid("bfloat16", "max") and not pico_amd.scale_valid("int32", "sum")
    assert _lib.PRIM_NAMES[7] == "SCALE" and _lib.PRIM_SCALED == 2
    leaves = (ctypes.c_void_p * 2)(None, None)
    for d, o in ((4, 0), (8, 5), (10, 10), (15, 0), (33, 4), (17, 0)):
        assert L.bine_reduce_tree_scaled(2, leaves, None, 16, d, o, 0, 0.5, None) == 1, (d, o)
        if (d, 0) not in good:
            assert L.bine_scale(None, None, 16, d, 0.5, None) == 1, d
    # op="avg" resolves in Python
    class C:
        size = 8
    assert pico_amd.api._scaled("avg", None, C) == ("sum", 0.125)
    assert pico_amd.api._scaled("max", 3.0, C) == ("max", 3.0)
    with pytest.raises(ValueError):
        pico_amd.api._scaled("avg", 2.0, C)
    assert "avg" not in pico_amd.OPS


# ---- 2. schedule identity -----------------------------------------------------------

def _pair(coll, algo, P, r, **kw):
    a = pico_amd.schedule(coll, algo, P, r, info=True, **kw)
    b = pico_amd.schedule(coll, algo, P, r, info=True, scaled=True, **kw)
    return a, b


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("form", list(FORMS))
def test_schedule_identity(P, form):
    """scaled schedule, flag cleared and SCALE removed == the unscaled one,
    entry for entry (ops, waits, c_join, workspace), uncut and with a chunk
    that cuts every block at least twice; in place and out of place.  A
    trailing SCALE comes last, on the caller's stream, and covers the rank's
    output; final_wait differs only where that SCALE already took the wait."""
    seen = 0
    for coll, algos in (("allreduce", AR), ("reduce_scatter", RS)):
        for algo in algos:
            per = 40
            rc = rcounts_of(algo, P, per) if coll == "reduce_scatter" else None
            count = per * P + 5
            for ip in (False, True):
                for chunk in (0, 4 * (per // 4)):   # 10 elements: at least 4 cuts of a 40-element block
                    kw = dict(count=count, rcounts=rc, esz=4, in_place=ip, chunk_bytes=chunk, **FORMS[form])
                    if not plans_ok(coll, algo, P, **kw):
                        continue
                    for r in range(P):
                        (ops, cj, fw, info), (sops, scj, sfw, sinfo) = _pair(coll, algo, P, r, **kw)
                        assert SS.strip(sops) == ops, (coll, algo, P, form, ip, chunk, r)
                        assert (cj, info) == (scj, sinfo)
                        scales = [(i, p) for i, o in enumerate(sops) for p in o["prims"] if p["type"] == "SCALE"]
                        flagged = [p for o in sops for p in o["prims"]
                                   if p["type"] == "REDUCE_TREE" and p["flags"] & _lib.PRIM_SCALED]
                        nout = rc[r] if rc else count
                        assert not (scales and flagged)
                        if scales:
                            assert len(scales) == 1 and scales[0][0] == len(sops) - 1 and not sops[-1]["xchg"]
                            p = scales[0][1]
                            assert (p["dst_buf"], p["dst_off"], p["count"]) == (1, 0, nout)
                            assert (p["src_buf"], p["src_off"]) == (1, 0)
                            assert sfw in (fw, -1)
                        else:
                            assert sfw == fw
                        seen += 1
    assert seen >= 8


# ---- 3. exactly once ------------------------------------------------------------------

def _small_ints(n, P):
    return [((np.arange(n) * 7 + 3 * r) % 11 + 1).astype(np.float32) for r in range(P)]


@pytest.mark.parametrize("P", PS)
def test_every_element_scaled_exactly_once(P):
    """fp32, small integer inputs, scale 3: x, 3x and 9x are all distinct and
    exact, so an element scaled twice or not at all shows.  Every rank's
    output of every form's replay == 3 x the literal unscaled replay."""
    ran = 0
    for coll, algos in (("allreduce", AR), ("reduce_scatter", RS)):
        for algo in algos:
            per = 13
            rc = rcounts_of(algo, P, per) if coll == "reduce_scatter" else None
            n = sum(rc) if rc else per * P + 5
            for ip in (False, True):
                base = dict(count=n, rcounts=rc, esz=4, in_place=ip)
                if not plans_ok(coll, algo, P, **base):
                    continue
                sb = _small_ints(n, P)
                want = SS.run(coll, algo, sb, "float", "sum", rcounts=rc, in_place=ip)
                assert all(np.all(w > 0) for w in want if w.size)
                for form, fk in FORMS.items():
                    for chunk in (0, 16):
                        got = SS.run(coll, algo, sb, "float", "sum", rcounts=rc, in_place=ip, chunk_bytes=chunk,
                                     scale=3.0, **fk)
                        for r in range(P):
                            assert np.array_equal(got[r], np.float32(3) * want[r]), (coll, algo, P, ip, form, chunk, r)
                        ran += 1
    assert ran


def test_multi_tree_mode_trails():
    """multi-tree mode (P = 4, 8): one trailing SCALE, no flag, 3x exactly"""
    for P in (4, 8):
        n = 4096 * P
        sb = _small_ints(n, P)
        want = SS.run("allreduce", "bine_bdw_remap", sb, "float", "sum")
        cnt = collections.Counter()
        got = SS.run("allreduce", "bine_bdw_remap", sb, "float", "sum", chunk_bytes=0, scale=3.0, trees=True,
                     flat_rs=True, counter=cnt)
        assert cnt["scale"] == P and cnt["tree"] == 0
        # (multi-tree mode reassociates: integer-valued fp32 sums are exact either way)
        for r in range(P):
            assert np.array_equal(got[r], np.float32(3) * want[r])


# ---- 4. fused, not appended --------------------------------------------------------------

@pytest.mark.parametrize("coll,algo", [("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_permute_remap")])
def test_fused_where_flat_trailing_where_literal(coll, algo):
    for P in (2, 4, 8):
        rc = [24] * P if coll == "reduce_scatter" else None
        for fk in (FORMS["flat_rs"], FORMS["flat_rs_ag1"], FORMS["flat_rs_ag2"]):
            for chunk in (0, 32):
                for ip in (False, True):
                    for r in range(P):
                        ops, _, _ = pico_amd.schedule(coll, algo, P, r, count=24 * P, rcounts=rc, esz=4, in_place=ip,
                                                      chunk_bytes=chunk, scaled=True, **fk)
                        prims = [p for o in ops for p in o["prims"]]
                        trees = [p for p in prims if p["type"] == "REDUCE_TREE"]
                        assert trees and all(p["flags"] & _lib.PRIM_SCALED for p in trees)
                        assert not [p for p in prims if p["type"] == "SCALE"]
                        if chunk:
                            assert len(trees) == 3   # 24 elements in chunks of 8: the copies inherit the flag
        for r in range(P):
            ops, _, _ = pico_amd.schedule(coll, algo, P, r, count=24 * P, rcounts=rc, esz=4, scaled=True)
            prims = [p for o in ops for p in o["prims"]]
            assert [p["type"] for p in prims].count("SCALE") == 1 and prims[-1]["type"] == "SCALE"
            assert not [p for p in prims if p["flags"] & _lib.PRIM_SCALED and p["type"] == "REDUCE_TREE"]


def test_ring_trails():
    """allreduce_ring at P = 3 (literal) and its flat form at P = 4 (the
    folded chain is no tree): exactly one trailing SCALE, no flag"""
    for P, fk in ((3, {}), (3, FORMS["flat_rs"]), (4, FORMS["flat_rs_ag1"])):
        for r in range(P):
            ops, _, _ = pico_amd.schedule("allreduce", "ring", P, r, count=50, esz=4, scaled=True, **fk)
            prims = [p for o in ops for p in o["prims"]]
            assert [p["type"] for p in prims].count("SCALE") == 1 and prims[-1]["type"] == "SCALE"
            assert not [p for p in prims if p["type"] == "REDUCE_TREE"]


def test_unscaled_schedule_has_neither():
    for coll, algo in (("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_send_remap")):
        for fk in FORMS.values():
            rc = [5, 6, 7, 5] if coll == "reduce_scatter" else None
            ops, _, _ = pico_amd.schedule(coll, algo, 4, 1, count=23, rcounts=rc, esz=2, chunk_bytes=8, **fk)
            assert not [p for o in ops for p in o["prims"] if p["type"] == "SCALE" or p["flags"] & _lib.PRIM_SCALED]
    with pytest.raises(pico_amd.BineError):   # bine_reduce has no scaled form
        pico_amd.schedule("reduce", "bine_bdw", 4, 0, count=64, scaled=True)


# ---- 5. the inputs expose the traps -----------------------------------------------------------

@pytest.mark.parametrize("dtype", H.TYPES)
def test_inputs_expose_single_rounding(dtype):
    """trap 1: S acts on the 16-bit reduced value.  On the GPU tests' P = 8 SUM
    inputs with scale 1/3, "scale the fp32 value of the last add, round once"
    differs from the specified result in at least one element"""
    n = 8195
    sb = H.inputs(dtype, n, 8, "sum")
    spec = SS.S(H.tree(sb, dtype, "sum"), dtype, 1 / 3)
    # the tree with its last level kept in fp32
    half = [H.tree(sb[:4], dtype, "sum"), H.tree(sb[4:], dtype, "sum")]
    last = H.to_f32(half[0], dtype) + H.to_f32(half[1], dtype)
    once = H.from_f32(last * np.float32(1 / 3), dtype)
    assert int((once != spec).sum()) >= 1
    # and the collective's replay agrees with the tree's definition
    lit = SS.run("allreduce", "bine_bdw_remap", sb, dtype, "sum")
    got = SS.run("allreduce", "bine_bdw_remap", sb, dtype, "sum", scale=1 / 3, chunk_bytes=4096, flat_rs=True,
                 flat_ag=2)
    for r in range(8):
        assert np.array_equal(got[r], SS.S(lit[r], dtype, 1 / 3))
        assert int((got[r] != lit[r]).sum()) > n // 2


def _toward_zero(x32, dtype):
    """float32 -> 16-bit by truncation (what a round-toward-zero conversion gives)"""
    x32 = np.ascontiguousarray(x32, np.float32)
    if dtype == "bfloat16":
        return (x32.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    with np.errstate(all="ignore"):
        near = x32.astype(np.float16)
        over = np.abs(near.astype(np.float32)) > np.abs(x32)     # rounded away from zero: step back
        bits = near.view(np.uint16).copy()
        bits[over] -= 1
        return bits


@pytest.mark.parametrize("dtype", H.TYPES)
def test_grid_exposes_truncation(dtype):
    """trap 2: on the special grid's values (and the random inputs), a final
    conversion that rounds toward zero differs from the specified result in
    at least one non-NaN element, for every scale the GPU tests use"""
    a, _ = H.special_grid(dtype)
    for s in (1 / 3, -0.1, 3.0):
        spec = SS.S(a, dtype, s)
        with np.errstate(all="ignore"):
            rz = _toward_zero(H.to_f32(a, dtype) * np.float32(s), dtype)
        ok = ~H.is_nan(spec, dtype)
        assert int((rz[ok] != spec[ok]).sum()) >= 1, (dtype, s)
    assert int((~H.is_nan(SS.S(a, dtype, 1 / 3), dtype)).sum()) >= 100


def test_S_matches_the_definition():
    """S() restated element by element for a few values per type"""
    for dtype in H.TYPES:
        x = H.random_bits(dtype, 64, 3)
        got = SS.S(x, dtype, -0.1)
        for k in range(x.size):
            v = np.float32(H.to_f32(x[k:k + 1], dtype)[0]) * np.float32(-0.1)
            assert got[k] == H.from_f32(np.array([v], np.float32), dtype)[0]
    x = np.array([1.0, 3.0, 1e-40, -7.5], np.float32)
    assert np.array_equal(SS.S(x, "float", 1 / 3), x * np.float32(1 / 3))
    assert SS.S(np.array([3.0]), "double", 1 / 3)[0] == 3.0 * (1 / 3)
