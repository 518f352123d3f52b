"""Wide (binary32-accumulating) reductions, host side: which path the planner
picks, the bit-5 schedules, the validity matrix, and the proof that the GPU
tests' inputs can tell a wide result from a plain 16-bit one."""
import numpy as np
import pytest

import h16_util as H
import plan_sim
import scale_sim as SS
import wide_sim as WS
import pico_amd
from pico_amd._lib import ALGOS, PRIM_SCALED, PRIM_WIDE, BineError

REDUCE_FAMILY = [("allreduce", a) for a in ALGOS["allreduce"]] + [("reduce_scatter", a) for a in ALGOS["reduce_scatter"]]
N = 4099


def counts(coll, P):
    return dict(count=N) if coll == "allreduce" else dict(rcounts=[N // P + (i % 3) for i in range(P)])


def scaled_fused(coll, algo, P, flat, trees):
    """whether the scaled plan's trees scale (Plan::scale_fused): flagged trees
    and no SCALE primitive; the plan's error status otherwise raised"""
    ops, _, _ = pico_amd.schedule(coll, algo, P, 0, esz=2, trees=trees, flat_ag=flat, flat_rs=flat, scaled=True,
                                  **counts(coll, P))
    prims = [p for o in ops for p in o["prims"]]
    flagged = any(p["type"] == "REDUCE_TREE" and p["flags"] & PRIM_SCALED for p in prims)
    trailing = any(p["type"] == "SCALE" for p in prims)
    assert flagged != trailing or not prims, (coll, algo, P, flat, trees)
    return flagged


@pytest.mark.parametrize("coll,algo", REDUCE_FAMILY)
def test_plan_wide_is_scale_fused(coll, algo):
    bad = []
    for P in range(1, 17):
        for flat in (False, True):
            for trees in (False, True):
                try:
                    want = scaled_fused(coll, algo, P, flat, trees)
                except BineError as e:
                    want = -e.status
                try:
                    got = pico_amd.wide_plan(coll, algo, P, trees=trees, flat_ag=flat, flat_rs=flat, **counts(coll, P))
                except BineError as e:
                    got = -e.status
                if got != want:
                    bad.append((P, flat, trees, got, want))
    assert not bad, bad[:8]


def test_plan_wide_takes_path_b_somewhere():
    assert pico_amd.wide_plan("allreduce", "bine_bdw_remap", 8, count=N, flat_rs=True, flat_ag=True) is True
    assert pico_amd.wide_plan("allreduce", "bine_lat", 4, count=N, flat_rs=True) is True
    assert pico_amd.wide_plan("reduce_scatter", "bine_permute_remap", 4, rcounts=[5] * 4, flat_rs=True) is True
    assert pico_amd.wide_plan("allreduce", "ring", 4, count=N, flat_rs=True) is False
    assert pico_amd.wide_plan("allreduce", "bine_bdw_remap", 8, count=N) is False
    assert pico_amd.wide_plan("allreduce", "bine_bdw_remap", 4, count=N, flat_rs=True, trees=True) is False
    assert pico_amd.wide_plan("allreduce", "bine_bdw_remap", 1, count=N, flat_rs=True) is False


def sched(coll, algo, P, r, **kw):
    return pico_amd.schedule(coll, algo, P, r, esz=2, chunk_bytes=4096, flat_ag=2, flat_rs=True, info=True,
                             **counts(coll, P), **kw)


@pytest.mark.parametrize("P", [2, 4, 8, 16])
def test_wide_schedules(P):
    """bit 5: the plain 16-bit schedule op for op and wait for wait, every final
    tree flagged; every output element covered by exactly one flagged tree"""
    seen_b = 0
    for coll, algo in REDUCE_FAMILY:
        kw = counts(coll, P)
        try:
            path_b = pico_amd.wide_plan(coll, algo, P, flat_ag=2, flat_rs=True, **kw)
        except BineError:
            continue
        if not path_b:
            with pytest.raises(BineError) as ei:
                sched(coll, algo, P, 0, wide=True)
            assert ei.value.status == 6, (coll, algo)   # BINE_ERR_UNSUPPORTED
            continue
        seen_b += 1
        total = np.zeros(N if coll == "allreduce" else 0, np.int64)
        for r in range(P):
            w, p = sched(coll, algo, P, r, wide=True), sched(coll, algo, P, r)
            assert w[1:] == p[1:], (coll, algo, r)
            assert len(w[0]) == len(p[0])
            nout = N if coll == "allreduce" else kw["rcounts"][r]
            cover = np.zeros(nout, np.int64)
            for ow, op_ in zip(w[0], p[0]):
                assert (ow["xchg"], ow["wait"]) == (op_["xchg"], op_["wait"])
                assert len(ow["prims"]) == len(op_["prims"])
                for a, b in zip(ow["prims"], op_["prims"]):
                    if a["type"] == "REDUCE_TREE":
                        assert a["flags"] & PRIM_WIDE and not a["flags"] & PRIM_SCALED, (coll, algo, r)
                        assert a["dst_buf"] == 1, (coll, algo, r)   # final: straight into RBUF
                        cover[a["dst_off"]:a["dst_off"] + a["count"]] += 1
                    assert dict(a, flags=a["flags"] & ~PRIM_WIDE) == b, (coll, algo, r)
            assert cover.max(initial=0) <= 1, (coll, algo, r)
            if coll == "reduce_scatter":
                assert (cover == 1).all(), (coll, algo, r)
            else:
                total += cover
        if coll == "allreduce":   # the ranks' blocks partition the output, or (one-shot) every rank computes all of it
            assert (total == 1).all() or (total == P).all(), (coll, algo, np.unique(total))
    assert seen_b >= 8
    with pytest.raises(BineError) as ei:   # scaled and wide together
        pico_amd.schedule("allreduce", "bine_bdw_remap", P, 0, esz=2, count=N, flat_rs=True, scaled=True, wide=True)
    assert ei.value.status == 1


def test_wide_valid_matrix():
    codes = list(range(17)) + [32, 33]
    assert len(codes) == 19
    L = pico_amd.lib()
    for d in codes + [17, 31, 34, -1]:
        for o in range(13):
            assert L.bine_wide_valid(d, o) == int(d in (32, 33) and o < 4), (d, o)
    assert pico_amd.wide_valid("bfloat16", "sum") and not pico_amd.wide_valid("float", "sum")


@pytest.mark.parametrize("dtype", H.TYPES)
def test_inputs_tell_wide_from_plain(dtype):
    """The GPU tests' inputs (h16_util.inputs under SUM, count 8195): the wide
    result differs from the plain 16-bit replay on some element -- with scale
    1.0 at every P >= 3.  At P = 2 one addition is all there is, and rounding
    its binary32 value once IS the correctly rounded 16-bit sum (and 1/2 is an
    exact scale), so no input can differ there under scale 1.0 or 1/P; the
    difference is shown under scale 1/3, where the plain call rounds twice.
    No expected element is non-finite (the cap elsewhere is 1/8)."""
    n = 8195
    for P in (2, 3, 4, 6, 8):
        sb = H.inputs(dtype, n, P, "sum")
        algo = "bine_bdw_remap" if P & (P - 1) == 0 else "ring"
        scale = 1 / 3 if P == 2 else 1.0
        wide = WS.collective("allreduce", algo, sb, dtype, "sum", scale=scale)
        with H.patched():
            plain = plan_sim.run("allreduce", algo, [x.copy() for x in sb], dtype, "sum")
        plain = [SS.S(x, dtype, scale) if scale != 1.0 else x for x in plain]
        assert any(not np.array_equal(w, p) for w, p in zip(wide, plain)), (dtype, P)
        f = H.to_f32(wide[0], dtype)
        assert np.isfinite(f).all(), (dtype, P)


@pytest.mark.parametrize("dtype", H.TYPES)
def test_wide_tree_rounds_once(dtype):
    """the host statement itself: 1 + u/2 + u/2 (u = ulp(1)) is 1 + u when
    accumulated in binary32 and 1 when every level rounds to 16 bits"""
    one, tie = H.specials(dtype)[5], H.specials(dtype)[11]
    leaves = [np.array([x], np.uint16) for x in (one, tie, tie, H.specials(dtype)[0])]
    assert WS.tree(leaves, dtype, "sum")[0] == H.specials(dtype)[10]
    assert H.tree(leaves, dtype, "sum")[0] == one
