"""Scaled (averaging) reductions on the GPU: bine_scale, the scaled tree and
the scaled collectives over loopback ranks on one GPU, against the host form
of S (tests/scale_sim.py) -- bit for bit wherever the expected value is not
NaN, NaN wherever it is.  Expected bits of the collectives: S(host replay of
the literal UNSCALED plan, tests/plan_sim.py), for the literal and the flat
forms alike."""
import numpy as np
import pytest

import h16_util as H
import plan_sim
import scale_sim as SS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)

TYPES = ["float", "double", "float16", "bfloat16"]
OPS4 = ["sum", "prod", "max", "min"]
SCALES = [0.125, 1 / 3, 3.0, -0.1]
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def esz_of(dtype):
    return np.dtype(SS.np_dtype(dtype)).itemsize


def shifted(arr, shift, pad=32):
    """a device byte buffer holding `arr` from element `shift` on; (tensor, address of the first element)"""
    e = arr.dtype.itemsize
    t = torch.zeros((arr.size + shift + pad) * e, dtype=torch.uint8, device="cuda:0")
    if arr.size:
        t[shift * e:(shift + arr.size) * e] = torch.from_numpy(arr.view(np.uint8).copy()).to("cuda:0")
    return t, t.data_ptr() + shift * e


def read(t, dtype, n, shift=0):
    e = esz_of(dtype)
    return t[shift * e:(shift + n) * e].cpu().numpy().view(SS.np_dtype(dtype)).copy()


def is_nan(x, dtype):
    return H.is_nan(x, dtype) if dtype in H.TYPES else np.isnan(x)


def same(got, exp, dtype):
    """bit-equal wherever exp is not NaN, NaN wherever it is"""
    if dtype in H.TYPES:
        return H.same(got, exp, dtype)
    if got.shape != exp.shape:
        return False
    nan = np.isnan(exp)
    u = UINT[got.dtype.itemsize]
    return bool(np.array_equal(got[~nan].view(u), exp[~nan].view(u)) and np.isnan(got[nan]).all())


def random_bits(dtype, n, seed):
    """random finite bit patterns of the type, subnormals included"""
    if dtype in H.TYPES:
        return H.random_bits(dtype, n, seed)
    rng = np.random.default_rng(seed)
    if dtype == "float":
        b = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        b = np.where((b & 0x7F800000) == 0x7F800000, b & np.uint32(0xFF7FFFFF), b).astype(np.uint32)
        return b.view(np.float32)
    b = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    m = np.uint64(0x7FF0000000000000)
    b = np.where((b & m) == m, b & ~np.uint64(0x0010000000000000), b).astype(np.uint64)
    return b.view(np.float64)


def inputs(dtype, n, P, op="sum", seed=1234):
    """per-rank inputs: H.inputs for the 16-bit types; for float / double the
    same classes (pico-like under SUM, near one under PROD, random bits under
    MAX / MIN)"""
    if dtype in H.TYPES:
        return H.inputs(dtype, n, P, op, seed)
    nd = SS.np_dtype(dtype)
    out = []
    for r in range(P):
        rng = np.random.default_rng(seed + r)
        if op == "sum":
            out.append((rng.random(n) * 100.0).astype(nd))
        elif op == "prod":
            out.append((rng.random(n) + 0.5).astype(nd))
        else:
            out.append(random_bits(dtype, n, seed + r))
    return out


def specials(dtype):
    """12 values: +-0, +-inf, NaN, +-1, two subnormals, the largest finite
    value, 1 + ulp, ulp(1) / 2"""
    if dtype in H.TYPES:
        return H.specials(dtype)
    nd = SS.np_dtype(dtype)
    fi = np.finfo(nd)
    tiny = fi.smallest_subnormal
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 3 * tiny, -(2 ** 20 + 1) * tiny, fi.max,
                     1.0 + fi.eps, fi.eps / 2], dtype=nd)


def value_of(x, dtype):
    """the double value of one element"""
    return float(H.to_f32(np.array([x], np.uint16), dtype)[0]) if dtype in H.TYPES else float(x)


# ---- bine_scale ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES)
def test_scale(dev, dtype):
    """every size class and the operand phases of test_reduce_local_and_reduce3
    ((1, 1) and (4, 4) co-aligned off a 16-B boundary, (1, 0) and (0, 3) not
    co-aligned), out of place and in place; nothing is written past the end"""
    for n in (1, 3, 7, 8, 9, 17, 1000, 100003):
        x = random_bits(dtype, n, 11 + n)
        if n == 1000:
            x = inputs(dtype, n, 1)[0]
        for k, (sa, sb) in enumerate(((0, 0), (1, 1), (1, 0), (0, 3), (4, 4))):
            for j, s in enumerate(SCALES):
                if n == 100003 and (j + k) % 4:   # the largest size: one scale per phase
                    continue
                exp = SS.S(x, dtype, s)
                ti, pi = shifted(x, sa)
                to, po = shifted(np.zeros(n, x.dtype), sb)
                pico_amd.scale(pi, po, n, dtype, s)
                tp, pp = shifted(x, sb)
                pico_amd.scale(pp, pp, n, dtype, s)   # in place
                torch.cuda.synchronize()
                assert same(read(to, dtype, n, sb), exp, dtype), (dtype, n, sa, sb, s, "out of place")
                assert same(read(tp, dtype, n, sb), exp, dtype), (dtype, n, sb, s, "in place")
                assert np.array_equal(read(ti, dtype, n, sa).view(np.uint8), x.view(np.uint8))   # input intact
                e = esz_of(dtype)
                assert not to[(sb + n) * e:(sb + n + 8) * e].any() and not tp[(sb + n) * e:(sb + n + 8) * e].any()
                assert not to[:sb * e].any()


@pytest.mark.parametrize("dtype", TYPES)
def test_scale_special_values(dev, dtype):
    """the 12 x 12 grid: element = special i, scale = the value of special j;
    through the vector body (16-B aligned, in place) and the scalar path (input
    one element off the output).  Non-NaN results bit for bit, NaN as NaN; at
    least 100 of the 144 results are not NaN"""
    v = specials(dtype)
    x = np.repeat(v, 12)          # 144 elements, so the body has full vectors
    non_nan = 0
    for j in range(12):
        s = value_of(v[j], dtype)
        exp = SS.S(x, dtype, s)
        non_nan += int((~is_nan(exp[::12], dtype)).sum())
        for sa, sb in ((0, 0), (1, 0)):
            ti, pi = shifted(x, sa)
            to, po = shifted(np.zeros(x.size, x.dtype), sb)
            pico_amd.scale(pi, po, x.size, dtype, s)
            torch.cuda.synchronize()
            got = read(to, dtype, x.size, sb)
            nan = is_nan(exp, dtype)
            u = UINT[esz_of(dtype)]
            assert np.array_equal(got[~nan].view(u), exp[~nan].view(u)), (dtype, j, sa, np.flatnonzero(
                (got.view(u) != exp.view(u)) & ~nan)[:8])
            assert is_nan(got[nan], dtype).all(), (dtype, j, sa)
    assert non_nan >= 100


# ---- bine_reduce_tree_scaled ---------------------------------------------------------------

def host_tree(leaves, dtype, op, swap):
    """level-by-level evaluation (bine_reduce_tree_swap): v[i] = v[i] (op) v[i + w], v[i] the inout side
    (v[i + w] where bit lvl of `swap` is set)"""
    if dtype in H.TYPES:
        return H.tree(leaves, dtype, op, swap)
    v = [np.array(x) for x in leaves]
    w, lvl = 1, 0
    while w < len(v):
        for i in range(0, len(v), 2 * w):
            if (swap >> lvl) & 1:
                t = v[i + w].copy()
                SS.reduce_local(v[i], t, dtype, op)
                v[i] = t
            else:
                SS.reduce_local(v[i + w], v[i], dtype, op)
        w *= 2
        lvl += 1
    return v[0]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("nl", [2, 4, 8, 16])
def test_reduce_tree_scaled(dev, dtype, nl):
    """the scaled tree == S(the unscaled tree's host evaluation): the four
    ops, swap masks 0 and 5, the scalar edges alone (n = 5) and the vector body
    with edges (n = 4099), leaves co-aligned with the output off a 16-B
    boundary and odd leaves one element off (the scalar kernel)"""
    k = 0
    for op in OPS4:
        for swap in (0, 5):
            for n in (5, 4099):
                for mis in (False, True):
                    s = (1 / 3, -0.1, 0.125, 3.0)[k % 4]
                    k += 1
                    host = inputs(dtype, n, nl, op, seed=300 + n)
                    want = SS.S(host_tree(host, dtype, op, swap), dtype, s)
                    leaves = [shifted(h, 3 + (1 if mis and j % 2 else 0)) for j, h in enumerate(host)]
                    to, po = shifted(np.zeros(n, host[0].dtype), 3)
                    assert pico_amd.reduce_tree([p for _, p in leaves], po, n, dtype, op, swap=swap, scale=s) == 0
                    torch.cuda.synchronize()
                    assert same(read(to, dtype, n, 3), want, dtype), (dtype, nl, op, swap, n, mis, s)
                    e = esz_of(dtype)
                    assert not to[(3 + n) * e:(3 + n + 8) * e].any()


# ---- collectives -----------------------------------------------------------------------------

N = 8195
CHUNK = 4096
POW2 = [("allreduce", "bine_bdw_remap"), ("allreduce", "bine_lat"), ("allreduce", "rabenseifner"),
        ("reduce_scatter", "bine_permute_remap"), ("reduce_scatter", "bine_send_remap")]
ODD = {3: [("allreduce", "ring")], 6: [("allreduce", "ring"), ("allreduce", "bine_block_by_block_any_even")]}


def rcounts_of(algo, P):
    per = N // P
    return [per + 1] * P if algo == "bine_permute_remap" else [per + (i % 3) for i in range(P)]


def to_dev(a, pad=64):
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.zeros(raw.size + pad, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t


def run(coll, algo, sb, dtype, op="sum", rc=None, in_place=False, scale=None, fill=0):
    """the collective on the loopback ranks; (per-rank outputs, statuses, the raw output tensors)"""
    P = len(sb)
    e = esz_of(dtype)
    ds = [to_dev(x) for x in sb]
    nout = rc if coll == "reduce_scatter" else [sb[0].size] * P
    dr = ds if in_place else [torch.full((max(c, 1) * e + 64,), fill, dtype=torch.uint8, device="cuda:0") for c in nout]
    torch.cuda.synchronize()
    src = [pico_amd.IN_PLACE] * P if in_place else ds
    if coll == "allreduce":
        _, st = pico_amd.loopback_allreduce(TG.comms(P), algo, src, dr, sb[0].size, dtype, op, scale=scale)
    else:
        _, st = pico_amd.loopback_reduce_scatter(TG.comms(P), algo, src, dr, rc, dtype, op, scale=scale)
    return [d[:c * e].cpu().numpy().view(SS.np_dtype(dtype)).copy() for d, c in zip(dr, nout)], st, dr


def literal(coll, algo, sb, dtype, op, rc, in_place):
    """host replay of the literal unscaled plan"""
    if dtype in H.TYPES:
        with H.patched():
            return plan_sim.run(coll, algo, [x.copy() for x in sb], dtype, op, rcounts=rc, in_place=in_place)
    return plan_sim.run(coll, algo, [x.copy() for x in sb], dtype, op, rcounts=rc, in_place=in_place)


def set_form(cs, flat):
    for c in cs:
        c.set_flat_rs(flat)
        c.set_flat_ag(2 if flat else 0)
        c.set_chunk(CHUNK if flat else 0)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("P", [1, 2, 3, 4, 6, 8])
def test_collectives(dev, P, dtype):
    """count 8195 (ragged for send_remap), scales 1/P and 1/3, the literal form
    and the flat one with the blocks cut (4 KiB chunks); in place once per
    type and P.  Expected: S(literal unscaled host replay), bit for bit"""
    bad = []
    cs = TG.comms(P)
    cache = {}
    try:
        for flat in (False, True):
            set_form(cs, flat)
            for i, (coll, algo) in enumerate(ODD.get(P, POW2)):
                rc = rcounts_of(algo, P) if coll == "reduce_scatter" else None
                n = sum(rc) if rc else N
                for ip in ((False, True) if i == 0 else (False,)):
                    key = (coll, algo, ip)
                    if key not in cache:   # one host replay serves both forms and both scales
                        sb = inputs(dtype, n, P, "sum")
                        cache[key] = (sb, literal(coll, algo, sb, dtype, "sum", rc, ip))
                    sb, lit = cache[key]
                    for s in (1.0 / P, 1 / 3):
                        if P == 1 and s == 1.0:
                            s = 3.0   # scale 1.0 is the unscaled path (tested below)
                        outs, st, _ = run(coll, algo, sb, dtype, "sum", rc, ip, s)
                        if any(st):
                            bad.append((coll, algo, flat, ip, s, "status", st))
                        elif not all(same(outs[r], SS.S(lit[r], dtype, s), dtype) for r in range(P)):
                            bad.append((coll, algo, flat, ip, s, "bits"))
    finally:
        set_form(cs, False)
    assert not bad, bad[:8]


@pytest.mark.parametrize("dtype", ["float", "bfloat16"])
def test_other_ops_scale_after_the_reduction(dev, dtype):
    """MAX and PROD, flat: S is applied after the reduction whatever the op"""
    P = 4
    cs = TG.comms(P)
    try:
        set_form(cs, True)
        for op in ("max", "prod"):
            sb = inputs(dtype, N, P, op)
            lit = literal("allreduce", "bine_bdw_remap", sb, dtype, op, None, False)
            outs, st, _ = run("allreduce", "bine_bdw_remap", sb, dtype, op, scale=-0.1)
            assert not any(st)
            assert all(same(outs[r], SS.S(lit[r], dtype, -0.1), dtype) for r in range(P)), (dtype, op)
    finally:
        set_form(cs, False)


def test_avg_and_unit_scale(dev):
    """op="avg" == op="sum", scale=1/P; scale=1.0 == the unscaled call's bits"""
    P = 4
    cs = TG.comms(P)
    try:
        for flat in (False, True):
            set_form(cs, flat)
            for dtype in ("float", "float16"):
                sb = inputs(dtype, N, P)
                plain, st0, _ = run("allreduce", "bine_bdw_remap", sb, dtype)
                unit, st1, _ = run("allreduce", "bine_bdw_remap", sb, dtype, scale=1.0)
                avg, st2, _ = run("allreduce", "bine_bdw_remap", sb, dtype, op="avg")
                quarter, st3, _ = run("allreduce", "bine_bdw_remap", sb, dtype, scale=0.25)
                assert not any(st0 + st1 + st2 + st3)
                for r in range(P):
                    assert unit[r].tobytes() == plain[r].tobytes()
                    assert avg[r].tobytes() == quarter[r].tobytes() == SS.S(plain[r], dtype, 0.25).tobytes()
            rc = rcounts_of("bine_send_remap", P)
            sb = inputs("double", sum(rc), P)
            a, sa, _ = run("reduce_scatter", "bine_send_remap", sb, "double", rc=rc, op="avg")
            b, sb_, _ = run("reduce_scatter", "bine_send_remap", sb, "double", rc=rc, scale=0.25)
            assert not any(sa + sb_) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        set_form(cs, False)


def test_one_rank_is_one_kernel(dev):
    """P = 1: out of place one out-of-place k_scale (not a copy plus a scale),
    in place one in-place k_scale -- one profiled op of 2 n esz bytes either way;
    at P = 4 flat the scaled call has exactly the ops of the unscaled one"""
    n = 100003
    c1 = TG.comms(1)
    x = inputs("float", n, 1)[0]
    try:
        c1[0].set_profile(True)
        for ip in (False, True):
            outs, st, _ = run("allreduce", "bine_bdw_remap", [x], "float", in_place=ip, scale=1 / 3)
            assert not any(st) and same(outs[0], SS.S(x, "float", 1 / 3), "float")
            prof = c1[0].profile()
            assert len(prof) == 1 and prof[0]["bytes"] == 2 * n * 4 and not prof[0]["xchg"], (ip, prof)
    finally:
        c1[0].set_profile(False)
    P = 4
    cs = TG.comms(P)
    sb = inputs("float", N, P)
    try:
        set_form(cs, True)
        for c in cs:
            c.set_profile(True)
        counts = []
        for s in (None, 1 / 3):
            _, st, _ = run("allreduce", "bine_bdw_remap", sb, "float", scale=s)
            assert not any(st)
            counts.append([(o["xchg"], o["nprims"], o["bytes"]) for o in cs[0].profile()])
        assert counts[0] == counts[1]   # a flagged tree's bytes are unchanged, and nothing is appended
    finally:
        for c in cs:
            c.set_profile(False)
        set_form(cs, False)


def test_invalid_pairs_are_refused(dev):
    """int32 sum scaled, float band scaled: BINE_ERR_ARG on every rank, rbuf untouched"""
    P, n = 2, 64
    cs = TG.comms(P)
    for dtype, op in (("int32", "sum"), ("float", "band"), ("c_float_complex", "sum")):
        sb = [np.arange(n * 2, dtype=np.int32) + r for r in range(P)]
        ds = [to_dev(x) for x in sb]
        dr = [torch.full((n * 8 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allreduce(cs, "bine_bdw_remap", ds, dr, n, dtype, op, scale=0.5)
        assert rc == 1 and st == [1] * P, (dtype, op, st)
        rc, st = pico_amd.loopback_reduce_scatter(cs, "bine_permute_remap", ds, dr, [n // 2] * P, dtype, op, scale=0.5)
        assert rc == 1 and st == [1] * P, (dtype, op, st)
        with pytest.raises(pico_amd.BineError) as ei:
            pico_amd.allreduce("bine_bdw_remap", ds[0], dr[0], n, dtype, op, cs[0], scale=0.5)
        assert ei.value.status == 1
        torch.cuda.synchronize()
        assert all(bool((d == 0x5A).all()) for d in dr), (dtype, op)
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.scale(ds[0], dr[0], n, "int32", 0.5)
    assert ei.value.status == 1
    assert pico_amd.reduce_tree([ds[0], ds[1]], dr[0], n, "float", "bor", scale=0.5) == 1
    torch.cuda.synchronize()
    assert bool((dr[0] == 0x5A).all())
