"""The case table of tools/dm_ops_check.py (the direct transport's in-launch
reductions on every type and op) means what it says -- proved on the CPU:
every row reaches the form it names on every rank (the planner's own
decisions, bine_plan_dm_fused / bine_plan_dm_trees at the transport's 1 MiB
slots), the table covers every (type, op) pair, vector count and workgroup
setting, and every row's inputs tell the right kernel from each plausible
wrong dispatch (another op, the sibling signedness, swapped operands)."""
import os
import sys

import numpy as np
import pytest

import pico_amd
import plan_sim
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dm_ops_check as D  # noqa: E402

RUNS = ((2, "small"), (2, "large"), (4, "small"), (4, "large"), (8, "large"), (3, "large"))
SINGLE_STREAM_BYTES = 1 << 20   # executor.cpp single_stream_bytes' default


def plans(row, P, rank):
    """(k_dm_fused launches as a small call, as a large call, hosting of every fused tree) by the
    planner; hosting: 'defer' (the next exchange), 'own' (the tree's own exchange), 'self' (a launch
    of its own)"""
    kw = dict(esz=D.ESZ[row.dtype], in_place=row.inplace, chunk_bytes=row.chunk, flat_ag=row.flat_ag, flat_rs=True)
    kw.update(dict(count=row.n) if row.coll == "allreduce" else dict(rcounts=[row.n] * P))
    pk = dict(kw, slot=D.SLOT, dtype=row.dtype, op=row.op)
    small = pico_amd.dm_fused_plan(row.coll, row.algo, P, rank, small=True, **pk)
    large = pico_amd.dm_fused_plan(row.coll, row.algo, P, rank, small=False, **pk)
    host, _ = pico_amd.dm_tree_plan(row.coll, row.algo, P, rank, **pk)
    ops, _, _ = pico_amd.schedule(row.coll, row.algo, P, rank, **kw)
    assert len(ops) == len(host)
    hosting = ["self" if h == j else "own" if h == ops[j]["wait"] else "defer" for j, h in enumerate(host) if h >= 0]
    return small, large, hosting


def form_of(row, P, rank, mode):
    """the form the executor gives the call (run_collective: single-stream calls try k_dm_fused
    with `single`; the others fused_for, then tree_plan_for -- both only with the fused trees on)"""
    small, large, hosting = plans(row, P, rank)
    nbytes = D.total_count(row, P) * D.ESZ[row.dtype]
    if mode == "small":
        assert nbytes <= SINGLE_STREAM_BYTES, row
        return ("small" if small == 1 else "fallback"), small, hosting
    if not row.tree:
        return "fallback", 0, []
    if large:
        return ("rs" if row.coll == "reduce_scatter" else "large"), large, hosting
    return ("tree" if hosting else "fallback"), 0, hosting


@pytest.mark.parametrize("P,mode", RUNS)
def test_every_row_reaches_its_form(P, mode):
    rows = D.cases(P, mode)
    assert rows
    seen = set()
    for row in rows:
        assert row.form in D.FORMS and row.wgs in D.WGS + (D.MIXED,) and row.tree in D.TREE_WGS + (0,), row
        for rank in range(P):
            form, launches, hosting = form_of(row, P, rank, mode)
            assert form == row.form, (row, rank, form, launches, hosting)
            if form == "rs":
                assert launches == D.launches_of(row), (row, launches)
            elif form == "large":
                assert launches == 1, (row, launches)
            if form == "tree":
                seen.update(hosting)
    if P in (2, 4) and mode == "large":
        # deferred trees, the last chunk's launch of its own, and (P > 2: at P = 2 the literal
        # allgather is the flat one) a tree inside its own exchange
        assert seen == ({"defer", "self", "own"} if P > 2 else {"defer", "self"}), seen
        assert {D.launches_of(r) for r in rows if r.form == "rs"} == {1, 2}
        nch = {r.n * D.ESZ[r.dtype] // r.chunk for r in rows if r.form == "rs"}
        assert nch == {1, 4, 6}, nch


def test_a_tree_row_the_one_launch_form_takes_is_noticed():
    """negative control: a `tree` row whose chunk grows to the whole block (one chunk and the flat
    allgather) is one k_dm_fused launch, and the form check says so"""
    row = next(r for r in D.cases(4, "large") if r.form == "tree" and r.flat_ag == 2)
    assert form_of(row, 4, 0, "large")[0] == "tree"
    assert form_of(row._replace(chunk=0), 4, 0, "large")[0] == "large"


def test_coverage():
    for P, mode, forms in ((2, "small", ("small",)), (2, "large", ("large", "tree")), (4, "small", ("small",)),
                           (4, "large", ("large", "tree")), (8, "large", ("large", "tree"))):
        rows = D.cases(P, mode)
        for form in forms:
            got = {(r.dtype, r.op) for r in rows if r.form == form}
            assert got == set(D.PAIRS), (P, mode, form, set(D.PAIRS) - got)
    for P, mode in ((2, "small"), (2, "large"), (4, "small"), (4, "large")):
        rows = D.cases(P, mode)
        for form in ("small",) if mode == "small" else ("large", "tree"):
            sel = [r for r in rows if r.form == form]
            nch = lambda r: max(1, (r.n // P) * D.ESZ[r.dtype] // r.chunk) if r.chunk else 1  # noqa: E731
            for pair in D.FULL + (None,):
                vs = {r.n * D.ESZ[r.dtype] // (16 * P * nch(r)) for r in sel if pair in (None, (r.dtype, r.op))}
                assert vs == set(D.VS), (P, mode, form, pair, vs)
            assert {r.wgs for r in sel} == set(D.WGS) | {D.MIXED}, (P, mode, form)
            if mode == "large":
                assert {r.tree for r in sel} == set(D.TREE_WGS), (P, mode, form)
            assert any(r.inplace for r in sel) and any(not r.inplace for r in sel)
        if mode == "large":
            assert any(r.form == "fallback" and r.tree == 0 for r in rows)
        assert any(r.form == "fallback" and r.tree and (r.n // P) * D.ESZ[r.dtype] % 16 for r in rows)
    assert {r.form for r in D.cases(3, "large")} == {"fallback"}
    assert D.environment("small").get("BINE_SINGLE_STREAM_BYTES") is None
    assert D.environment("large")["BINE_SINGLE_STREAM_BYTES"] == "0"
    assert D.environment("large")["BINE_DIRECT_TREE_WGS"] == "1"   # set_direct_tree(1): one tree workgroup


SIBLING = {"int32": "uint32", "uint32": "int32", "int64": "uint64", "uint64": "int64"}


def _swapped(monkeypatch, row, P, sb):
    """the literal schedule replayed with every reduction's operands swapped (the flat trees keep
    the literal schedule's operand order, so this is comb16(r, l) throughout)"""
    real = O.reduce_local

    def swapped(inp, inout, dtype, op="sum"):
        a = inp.copy()
        real(np.ascontiguousarray(inout), a, dtype, op)   # inp as the inout side
        inout[:] = a

    with monkeypatch.context() as m:
        m.setattr(O, "reduce_local", swapped)
        return plan_sim.run(row.coll, row.algo, [x.copy() for x in sb], row.dtype, row.op,
                            rcounts=[row.n] * P if row.coll == "reduce_scatter" else None)


def _bytes(outs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in outs)


@pytest.mark.parametrize("P,mode", RUNS)
def test_rows_tell_wrong_dispatches_apart(P, mode, monkeypatch):
    """every row's expected output differs from what its inputs give under another op, under the
    sibling signedness (MAX / MIN: two's-complement SUM and PROD have the same bits for both, so no
    input can tell them apart) and, floating MAX / MIN, under swapped operands (signed zeros, the
    NaN's position; IEEE SUM and PROD commute bit for bit with one NaN encoding, so there the swap
    must NOT show -- checked, as the control of the replay)"""
    done = set()
    for index, row in enumerate(D.cases(P, mode)):
        sb = D.inputs(row, P, D.seed_of(index))
        want = _bytes(D.expected(row, P, sb))
        key = (row.coll, row.algo, row.dtype, row.op, row.n)
        for op in D.OPS:
            if op != row.op:
                assert _bytes(D.expected(row._replace(op=op), P, sb)) != want, (row, op)
        if row.dtype in SIBLING and row.op in ("max", "min"):
            sib = SIBLING[row.dtype]
            other = D.expected(row._replace(dtype=sib), P, [x.view(O.NP_DTYPES[sib]) for x in sb])
            assert _bytes(other) != want, (row, sib)
        if row.dtype in ("float", "double") and key not in done and (row.op in ("max", "min") or row.n <= 64 * P):
            done.add(key)
            assert _bytes(plan_sim.run(row.coll, row.algo, [x.copy() for x in sb], row.dtype, row.op,
                                       rcounts=[row.n] * P if row.coll == "reduce_scatter" else None)) == want
            sw = _bytes(_swapped(monkeypatch, row, P, sb))
            assert (sw != want) == (row.op in ("max", "min")), (row, "swapped operands")


@pytest.mark.parametrize("P,mode", RUNS)
def test_inputs_stay_finite_outside_the_planted_values(P, mode):
    """floating SUM / PROD rows: outside the planted specials at most 1/8 of the expected elements are
    non-finite (the magnitudes: 8 ranks' products and sums stay in range), so the bit-exact comparison
    is of numbers, not of NaNs; and the planted ones do produce NaN, inf, -0.0 and denormals"""
    kinds = set()
    for index, row in enumerate(D.cases(P, mode)):
        if row.dtype not in ("float", "double"):
            continue
        sb = D.inputs(row, P, D.seed_of(index))
        for r, x in enumerate(D.expected(row, P, sb)):
            n = x.size
            # rank r's output block starts at element r * n of the input for a reduce-scatter
            pl = D.planted(D.total_count(row, P))[(r * n if row.coll == "reduce_scatter" else 0):][:n]
            if row.op in ("sum", "prod"):
                rest = x[~pl]
                assert (~np.isfinite(rest)).sum() * 8 <= rest.size, (row, r)
            tiny = np.finfo(x.dtype).tiny
            kinds.update(k for k, m in (("nan", np.isnan(x)), ("inf", np.isinf(x)), ("-0", (x == 0) & np.signbit(x)),
                                        ("denormal", (x != 0) & (np.abs(x) < tiny))) if m[pl].any())
    if any(r.dtype in ("float", "double") for r in D.cases(P, mode)):
        assert kinds == {"nan", "inf", "-0", "denormal"}, kinds
