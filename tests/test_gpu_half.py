"""float16 / bfloat16 on the GPU: the reduction kernels (pairwise, batched,
tree) and every reduce-family collective over loopback ranks on one GPU,
against the host arithmetic of tests/h16_util.py -- bit for bit wherever the
expected value is not NaN, NaN wherever it is (a NaN's payload is
unspecified).  Expected bits of the collectives: the host replay of the
literal plan (tests/plan_sim.py), for the literal and the flat forms alike."""
import numpy as np
import pytest

import h16_util as H
import plan_sim

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the loopback drivers and the communicator cache)

OPS4 = ["sum", "prod", "max", "min"]
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def shifted(bits, shift, pad=32):
    """a device byte buffer holding `bits` from element `shift` on; returns
    (tensor, address of the first element)"""
    t = torch.zeros((bits.size + shift + pad) * 2, dtype=torch.uint8, device="cuda:0")
    if bits.size:
        t[shift * 2:(shift + bits.size) * 2] = torch.from_numpy(bits.view(np.uint8).copy()).to("cuda:0")
    return t, t.data_ptr() + shift * 2


def bits_of(t, n, shift=0):
    return t[shift * 2:(shift + n) * 2].cpu().numpy().view(np.uint16).copy()


# ---- the arithmetic boundary ---------------------------------------------------

@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("op", OPS4)
def test_reduce_local_and_reduce3(dev, dtype, op):
    """every size class (scalar only, head + body + tail, several tiles) and
    operand phase: (1, 1) and (4, 4) co-aligned off a 16-B boundary, (1, 0) and
    (0, 3) not co-aligned -- odd shifts give 2-byte-aligned operands"""
    for n in (1, 3, 7, 8, 9, 17, 1000, 100003):
        for sa, sb in ((0, 0), (1, 1), (1, 0), (0, 3), (4, 4)):
            a, b = H.random_bits(dtype, n, 11 + n), H.random_bits(dtype, n, 97 + n)
            if op in ("sum", "prod") and n == 1000:
                a, b = H.inputs(dtype, n, 2, op)
            exp = b.copy()
            H.reduce_local(a, exp, dtype, op)
            ta, pa = shifted(a, sa)
            tb, pb = shifted(b, sb)
            to, po = shifted(np.zeros(n, np.uint16), sb)
            pico_amd.reduce3(pa, pb, po, n, dtype, op)
            pico_amd.reduce_local(pa, pb, n, dtype, op)
            torch.cuda.synchronize()
            assert H.same(bits_of(tb, n, sb), exp, dtype), (dtype, op, n, sa, sb, "reduce_local")
            assert H.same(bits_of(to, n, sb), exp, dtype), (dtype, op, n, sa, sb, "reduce3")
            assert not bits_of(tb, 8, sb + n).any() and not bits_of(to, 8, sb + n).any()   # nothing past the end


@pytest.mark.parametrize("dtype", H.TYPES)
def test_torch_tensors_resolve_their_dtype(dev, dtype):
    """reduce_local on torch.float16 / torch.bfloat16 tensors (dtype=None)"""
    n = 4099
    a, b = H.inputs(dtype, n, 2, "sum")
    ta = torch.from_numpy(a.view(np.int16).copy()).to(dev).view(TORCH_DT[dtype])
    tb = torch.from_numpy(b.view(np.int16).copy()).to(dev).view(TORCH_DT[dtype])
    pico_amd.reduce_local(ta, tb, n, None, "sum")
    torch.cuda.synchronize()
    exp = b.copy()
    H.reduce_local(a, exp, dtype, "sum")
    assert np.array_equal(tb.view(torch.int16).cpu().numpy().view(np.uint16), exp)


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("op", OPS4)
def test_special_values(dev, dtype, op):
    """the 12 x 12 grid (+-0, +-inf, NaN, +-1, subnormals, the largest finite
    value, 1 + ulp, a rounding tie): NaN-class results as NaN, all others --
    at least 100 of the 144 -- bit for bit, through the vector body (the grid
    16-B aligned) and the scalar path (off by one element)"""
    a, b = H.special_grid(dtype)
    exp = b.copy()
    H.reduce_local(a, exp, dtype, op)
    nan = H.is_nan(exp, dtype)
    assert nan.sum() <= 31 and (~nan).sum() >= 100
    for sa, sb in ((0, 0), (1, 0)):
        ta, pa = shifted(a, sa)
        tb, pb = shifted(b, sb)
        pico_amd.reduce_local(pa, pb, a.size, dtype, op)
        torch.cuda.synchronize()
        got = bits_of(tb, a.size, sb)
        assert np.array_equal(got[~nan], exp[~nan]), (dtype, op, sa, np.flatnonzero((got != exp) & ~nan)[:8])
        assert H.is_nan(got[nan], dtype).all(), (dtype, op, sa)


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("nl", [2, 4, 8, 16])
def test_reduce_tree(dev, dtype, nl):
    """bine_reduce_tree against the level-by-level host evaluation (every
    level rounds to the 16-bit type): swap masks 0 and 5, the scalar edges
    alone (n = 5) and the vector body with edges (n = 4099), leaves co-aligned
    with the output off a 16-B boundary and odd leaves one element off"""
    for op in OPS4:
        for swap in (0, 5):
            for n in (5, 4099):
                for mis in (False, True):
                    host = H.inputs(dtype, n, nl, op, seed=300 + n)
                    want = H.tree(host, dtype, op, swap)
                    leaves = [shifted(h, 3 + (1 if mis and j % 2 else 0)) for j, h in enumerate(host)]
                    to, po = shifted(np.zeros(n, np.uint16), 3)
                    assert pico_amd.reduce_tree([p for _, p in leaves], po, n, dtype, op, swap=swap) == 0
                    torch.cuda.synchronize()
                    assert H.same(bits_of(to, n, 3), want, dtype), (dtype, nl, op, swap, n, mis)
                    assert not bits_of(to, 8, 3 + n).any()


@pytest.mark.parametrize("dtype", H.TYPES)
def test_reduce_batch(dev, dtype):
    """3 windows of different lengths in one launch"""
    for op in OPS4:
        counts = [5, 1000, 4099]
        ins = [H.inputs(dtype, n, 1, op, seed=40 + n)[0] for n in counts]
        ios = [H.inputs(dtype, n, 1, op, seed=80 + n)[0] for n in counts]
        ti = [shifted(x, 0) for x in ins]
        tio = [shifted(x, 0) for x in ios]
        assert pico_amd.reduce_batch([p for _, p in ti], [p for _, p in tio], counts, dtype, op) == 0
        torch.cuda.synchronize()
        for k, n in enumerate(counts):
            exp = ios[k].copy()
            H.reduce_local(ins[k], exp, dtype, op)
            assert H.same(bits_of(tio[k][0], n), exp, dtype), (dtype, op, k)


# ---- collectives -----------------------------------------------------------------

FAMILIES = {"allreduce": sorted(pico_amd.ALGOS["allreduce"]), "reduce_scatter": sorted(pico_amd.ALGOS["reduce_scatter"]),
            "reduce": sorted(pico_amd.ALGOS["reduce"])}
EXTRA_OPS = {"allreduce": "bine_bdw_remap", "reduce_scatter": "bine_static", "reduce": "bine_bdw"}
SEG = 4096


def expected(coll, algo, sb, dtype, op, rc, in_place):
    """(per-rank statuses from the plan, per-rank bits from the host replay of
    the literal plan); bits None where some rank refuses"""
    P = len(sb)
    st = []
    for r in range(P):
        try:
            pico_amd.plan(coll, algo, P, r, count=sb[0].size, rcounts=rc, esz=2, segsize=SEG, in_place=in_place)
            st.append(0)
        except pico_amd.BineError as e:
            st.append(e.status)
    if any(st):
        return st, None
    return st, plan_sim.run(coll, algo, [x.copy() for x in sb], dtype, op, rcounts=rc, segsize=SEG, in_place=in_place)


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("P", [2, 3, 4, 6, 8])
@pytest.mark.parametrize("coll", list(FAMILIES))
def test_collectives(dev, coll, P, dtype):
    """every algorithm of the family, counts 3P + 5 and 1024P + 3 (the second
    in place), the literal form and the flat one; SUM everywhere, MAX and PROD
    on one algorithm"""
    bad = []
    cs = TG.comms(P)
    cache = {}
    with H.patched():
        try:
            for flat in (False, True):
                for c in cs:
                    c.set_flat_rs(flat)
                    c.set_flat_ag(2 if flat else 0)
                    c.set_chunk(4096 if flat else 0)
                for algo in FAMILIES[coll]:
                    for op in ["sum"] + (["max", "prod"] if algo == EXTRA_OPS[coll] else []):
                        for n, ip in ((3 * P + 5, False), (1024 * P + 3, True)):
                            rc = None
                            if coll == "reduce_scatter":
                                rc = [n // P + 1] * P if algo == "bine_permute_remap" else \
                                    [n // P + (i % 3) for i in range(P)]
                            key = (algo, op, n)
                            if key not in cache:   # one host replay serves both forms
                                sb = H.inputs(dtype, sum(rc) if rc else n, P, op)
                                cache[key] = (sb,) + expected(coll, algo, sb, dtype, op, rc, ip)
                            sb, est, want = cache[key]
                            outs, st = TG.run_loopback(coll, algo, sb, dtype, op, rcounts=rc, segsize=SEG, in_place=ip)
                            if st != est:
                                bad.append((algo, op, n, flat, "status", st, est))
                            elif want is not None:
                                ranks = [0] if coll == "reduce" else range(P)
                                if not all(H.same(outs[r], want[r], dtype) for r in ranks):
                                    bad.append((algo, op, n, flat, "bits"))
        finally:
            for c in cs:
                c.set_flat_rs(False)
                c.set_flat_ag(False)
                c.set_chunk(0)
    assert not bad, bad[:8]


def test_data_movement_carries_them_as_two_byte_types(dev):
    """allgather, bcast and alltoall with "bfloat16" deliver the bytes they
    deliver with "uint16" """
    P, n = 4, 1027
    with H.patched():
        for coll, algo, total in (("allgather", "bine_send_remap", n), ("bcast", "bine_lat", n),
                                  ("alltoall", "bine", n * P)):
            sb = [H.random_bits("bfloat16", total, 500 + r) for r in range(P)]
            a, sa = TG.run_loopback(coll, algo, sb, "bfloat16")
            b, sb_ = TG.run_loopback(coll, algo, sb, "uint16")
            assert sa == sb_ == [0] * P, (coll, sa, sb_)
            assert all(x.tobytes() == y.tobytes() and x.size for x, y in zip(a, b)), coll
            if coll == "bcast":
                assert all(x.tobytes() == sb[0].tobytes() for x in a)


def test_checksum_reads_two_byte_elements(dev):
    a = H.random_bits("float16", 123457, 5)
    t, _ = shifted(a, 0)
    assert pico_amd.checksum(t, a.size, "float16") == pico_amd.checksum(t, a.size, "uint16") == TG.host_checksum(a)
    assert pico_amd.checksum(t, a.size, "bfloat16") == TG.host_checksum(a)


def test_undefined_ops_are_refused(dev):
    """bitwise / logical / loc ops on the 16-bit floating types: BINE_ERR_ARG
    on every rank, before any exchange"""
    P, n = 2, 64
    cs = TG.comms(P)
    s = [torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(P)]
    r = [torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(P)]
    torch.cuda.synchronize()
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.allreduce("bine_bdw_remap", s[0], r[0], n, "bfloat16", "band", cs[0])
    assert ei.value.status == 1 and pico_amd._lib.STATUS[1] == "ERR_ARG"
    for op in ("band", "lor", "maxloc"):
        rc, st = pico_amd.loopback_allreduce(cs, "bine_bdw_remap", s, r, n, None, op)
        assert st == [1] * P, (op, st)
        with pytest.raises(pico_amd.BineError) as ei:
            pico_amd.reduce_local(s[0], r[0], n, "float16", op)
        assert ei.value.status == 1
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.fill_pico(s[0], n, "bfloat16")
    assert ei.value.status == 6   # ERR_UNSUPPORTED: pico_core has no such distribution
