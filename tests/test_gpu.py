"""GPU parity tests: the HIP path (libbine_amd.so through its C ABI) against the
reference's own golden vectors and the oracle.  Bit-exact for every dtype: the
schedule fixes the per-element association order, and the kernels reproduce
MPICH's IEEE arithmetic (fp32/fp64 tolerance used: 0 ulp).

Multi-rank cases run on ONE GPU through the loopback transport (virtual ranks,
in-process peer copies); the RCCL transport is exercised at P = 1 here, in
real processes by tests/test_gpu_rccl.py, and over xGMI by the driver's
multi-GPU bench.
"""
import hashlib
import os

import numpy as np
import pytest

import _sub
import golden_util as G
import rooted_util as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_DT = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float", "double"]
STATUS_OF_MPI = {12: 1, 51: 2, 7: 8, 2: 9}   # MPI_ERR_ARG / _SIZE / _ROOT / _COUNT -> BINE_ERR_*


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def to_dev(a: np.ndarray, pad: int = 0):
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.zeros(raw.size + pad, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[: raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t


def from_dev(t, dtype: str, n: int, off_bytes: int = 0) -> np.ndarray:
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    raw = t[off_bytes: off_bytes + n * esz].cpu().numpy()
    return raw.view(O.NP_DTYPES[dtype]).copy()


def sha(a):
    return hashlib.sha256(O.canonical(np.asarray(a))).hexdigest()   # pair types: padding zeroed


# ---- the arithmetic boundary -------------------------------------------------------

@pytest.mark.parametrize("dtype", ALL_DT)
@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
def test_reduce_local_bit_exact(dev, dtype, op):
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    for n in (1, 3, 17, 1000, 100003):
        for shift_a, shift_b in ((0, 0), (1, 1), (1, 0), (0, 3)):
            a = O.fill(dtype, n, 11 + n)
            b = O.fill(dtype, n, 97 + n)
            ta = to_dev(np.concatenate([np.zeros(shift_a, a.dtype), a]))
            tb = to_dev(np.concatenate([np.zeros(shift_b, b.dtype), b]), pad=64)
            pico_amd.reduce_local(ta.data_ptr() + shift_a * esz, tb.data_ptr() + shift_b * esz, n, dtype, op)
            torch.cuda.synchronize()
            exp = b.copy()
            O.reduce_local(a, exp, dtype, op)
            raw = tb.cpu().numpy()
            got = raw[shift_b * esz:(shift_b + n) * esz]
            assert got.tobytes() == exp.tobytes(), (dtype, op, n, shift_a, shift_b)
            # the elements before inout and the 64 bytes past it stay zero
            assert not raw[:shift_b * esz].any() and not raw[(shift_b + n) * esz:].any(), (dtype, op, n, shift_b)


@pytest.mark.parametrize("dtype", ["float", "double"])
@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
def test_reduce_local_special_values(dev, dtype, op):
    npdt = O.NP_DTYPES[dtype]
    tiny = np.finfo(npdt).tiny
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, tiny / 4, -tiny / 8, 3e38 if dtype == "float" else 1e300],
                    dtype=npdt)
    a = np.repeat(vals, vals.size)
    b = np.tile(vals, vals.size)
    ta, tb = to_dev(a), to_dev(b)
    pico_amd.reduce_local(ta, tb.data_ptr(), a.size, dtype, op)
    torch.cuda.synchronize()
    exp = b.copy()
    O.reduce_local(a, exp, dtype, op)
    assert from_dev(tb, dtype, a.size).tobytes() == exp.tobytes()   # NaN payloads, signed zeros, denormals


def test_reduce3_out_of_place(dev):
    a, b = O.fill("float", 5003, 1), O.fill("float", 5003, 2)
    ta, tb, to = to_dev(a), to_dev(b), to_dev(np.zeros_like(a))
    pico_amd.reduce3(ta, tb, to, a.size, "float", "sum")
    torch.cuda.synchronize()
    exp = b.copy()
    O.reduce_local(a, exp, "float")
    assert from_dev(to, "float", a.size).tobytes() == exp.tobytes()
    assert from_dev(tb, "float", a.size).tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", ALL_DT)
def test_fill_pico_matches_host_generator(dev, dtype):
    for n, seed in ((1, 1234), (1000, 1235), (70001, 99)):
        esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
        t = torch.zeros(n * esz, dtype=torch.uint8, device=dev)
        pico_amd.fill_pico(t, n, dtype, seed)
        torch.cuda.synchronize()
        assert from_dev(t, dtype, n).tobytes() == O.fill(dtype, n, seed).tobytes(), (dtype, n)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def host_checksum(a: np.ndarray) -> int:
    bits = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.uint64)
    idx = np.arange(a.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        return int(_mix64(bits + idx).sum(dtype=np.uint64))


def test_checksum_matches_host(dev):
    for dtype in ("float", "int64", "int8"):
        a = O.fill(dtype, 123457, 5)
        assert pico_amd.checksum(to_dev(a), a.size, dtype) == host_checksum(a)


# ---- collectives vs the reference's golden vectors (loopback ranks) ----------------

_COMMS = {}


def comms(P):
    if P not in _COMMS:
        _COMMS[P] = pico_amd.Comm.loopback(P, 0)
    return _COMMS[P]


def run_loopback(coll, algo, sbufs, dtype, op="sum", rcounts=None, segsize=0, root=0, in_place=False, relay=0):
    P = len(sbufs)
    for c in comms(P):
        c.set_relay(relay)
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    n = sbufs[0].size
    ds = [to_dev(x, pad=64) for x in sbufs]
    if coll == "allreduce":
        dr = ds if in_place else [torch.zeros(n * esz + 64, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allreduce(comms(P), algo, [pico_amd.IN_PLACE] * P if in_place else ds, dr, n,
                                             dtype, op, segsize)
        outs = [from_dev(d, dtype, n) for d in dr]
    elif coll == "reduce_scatter":
        dr = ds if in_place else [torch.zeros(max(c, 1) * esz + 64, dtype=torch.uint8, device="cuda:0") for c in rcounts]
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_reduce_scatter(comms(P), algo, [pico_amd.IN_PLACE] * P if in_place else ds, dr,
                                                  rcounts, dtype, op)
        outs = [from_dev(d, dtype, c) for d, c in zip(dr, rcounts)]
    elif coll == "allgather":
        dr = [torch.zeros(P * n * esz + 64, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
        if in_place:   # MPI_IN_PLACE: the own block already at block r of rbuf
            for r in range(P):
                dr[r][r * n * esz:(r + 1) * n * esz] = ds[r][:n * esz]
            ds = [pico_amd.IN_PLACE] * P
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allgather(comms(P), algo, ds, dr, n, dtype)
        outs = [from_dev(d, dtype, P * n) for d in dr]
    elif coll == "bcast":   # in place: every rank's buffer holds its input
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_bcast(comms(P), algo, ds, n, dtype, root)
        outs = [from_dev(d, dtype, n) for d in ds]
    elif coll in R.ROOTED:
        # n = elements per block; gather: rbuf on the root only, scatter: sbuf
        # on the root only (the others pass NULL, as pico_core does)
        n = n if coll == "gather" else n // P
        rn = [P * n if (coll != "gather" or r == root) and coll != "scatter" else n if coll == "scatter" else 0
              for r in range(P)]
        dr = [torch.zeros(k * esz + 64, dtype=torch.uint8, device="cuda:0") if k else None for k in rn]
        if coll == "scatter":
            ds = [d if r == root else None for r, d in enumerate(ds)]
        torch.cuda.synchronize()
        if coll == "alltoall":
            rc, st = pico_amd.loopback_alltoall(comms(P), algo, ds, dr, n, dtype)
        else:
            fn = pico_amd.loopback_gather if coll == "gather" else pico_amd.loopback_scatter
            rc, st = fn(comms(P), algo, ds, dr, n, dtype, root)
        outs = [from_dev(d, dtype, k) if k else np.zeros(0, O.NP_DTYPES[dtype]) for d, k in zip(dr, rn)]
    else:
        dr = [torch.zeros(n * esz + 64, dtype=torch.uint8, device="cuda:0") if r == root else None for r in range(P)]
        if in_place:   # MPI_IN_PLACE at the root: its input already sits in its receive buffer
            dr[root] = ds[root]
            ds = [pico_amd.IN_PLACE if r == root else d for r, d in enumerate(ds)]
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_reduce(comms(P), algo, ds, dr, n, dtype, op, root)
        outs = [from_dev(dr[root], dtype, n)] + [np.zeros(0)] * (P - 1)
    return outs, st


def oracle_bcast(algo, sb, dt, root):
    """(outputs, rets) the device path must give for a bcast: the oracle's
    replay; where the reference crashes, the root's buffer everywhere
    (scatter_allgather's wrapped counts) or MPI_ERR_ARG (bine_bdw_remap off
    root 0 / a power-of-two P, where it asserts) -- DESIGN.md deviations"""
    if algo not in O.BC_BDW:
        return O.bcast(algo, sb, dt, root)
    out, rets = O.bcast_bdw(algo, sb, dt, root)
    if rets and rets[0] == "crash":
        if algo == "bine_bdw_remap":
            return [np.array(b).copy() for b in sb], [O.ERR_ARG] * len(sb)
        return [np.array(sb[root]).copy() for _ in sb], [0] * len(sb)
    return out, rets


def in_place_rbufs(sb, dt):
    """allgather with MPI_IN_PLACE: every rank's rbuf holding its own block"""
    P, n = len(sb), sb[0].size
    out = []
    for r in range(P):
        b = np.zeros(P * n, O.NP_DTYPES[dt])
        b[r * n:(r + 1) * n] = sb[r]
        out.append(b)
    return out


def oracle_outputs(coll, algo, sb, dt, op, rk, segsize, root=0, in_place=False):
    """the oracle's per-rank outputs of one collective (intended semantics:
    the reference's bugs are not reproduced)"""
    if coll == "bcast":
        return oracle_bcast(algo, sb, dt, root)[0]
    if coll == "allgather":
        return O.allgather(algo, sb, dt, in_place_rbufs=in_place_rbufs(sb, dt) if in_place else None)[0]
    if coll == "reduce_scatter":
        return O.reduce_scatter(algo, sb, rk, dt, op)[0]
    if coll == "reduce":
        return [O.reduce(algo, sb, dt, op)[0]]
    return O.allreduce(algo, sb, dt, op, segsize, ref_bugs=False)[0]


def _golden_groups():
    g = {}
    for c in G.cases():
        if c["coll"] == "fill" or c["N"] > 300000:
            continue
        g.setdefault((c["coll"], c["algo"]), []).append(c)
    return sorted(g.items())


@pytest.mark.parametrize("relay", [0, 16], ids=["direct", "relay"])
@pytest.mark.parametrize("key,cs", _golden_groups(), ids=lambda x: ".".join(x) if isinstance(x, tuple) else "")
def test_collectives_match_reference_goldens(dev, key, cs, relay):
    """relay: the same cases with the multi-link relay schedule (two-hop
    routes through the other ranks) -- results must not change a bit (the
    segmented algorithm's relay pass skips the cases of more than 512
    segments: up to 32,768 segments a case, 90 of the suite's seconds, for
    the same relay routes its smaller cases take)."""
    coll, algo = key
    bad = []
    for c in cs:
        P, N, dt = c["P"], c["N"], c["dtype"]
        if relay and P < 3:
            continue
        rk = G.rcounts(c) if coll == "reduce_scatter" else None
        sb = G.inputs(c, sum(rk) if rk else N * P if coll in ("scatter", "alltoall") else N)
        if coll in R.ROOTED:
            # the reference's result where it delivers the collective, else the
            # product's refusal (tests/rooted_util.py)
            root = G.root(c)
            want, exp = R.expect(coll, sb, dt, root, P, N)
            outs, st = run_loopback(coll, algo, sb, dt, root=root, relay=relay)
            if st != [exp] * P:
                bad.append((c["id"], "status", st, exp))
            elif not exp and c["status"] == "ok" and G.check_rank_outputs(c, outs):
                bad.append((c["id"], "ranks"))
            elif not exp and any(O.canonical(o) != (b"" if w is None else O.canonical(w)) for o, w in zip(outs, want)):
                bad.append((c["id"], "vs-oracle"))
            continue
        if relay and c["segsize"] and N * sb[0].itemsize > 512 * c["segsize"]:
            continue
        ip = c["rcounts"].endswith("_inplace")   # MPI_IN_PLACE cases (the reference's in-place paths)
        root = G.root(c) if coll == "bcast" else 0
        outs, st = run_loopback(coll, algo, sb, dt, c["op"], rk, c["segsize"], root=root, relay=relay, in_place=ip)
        if coll == "allgather" and c["status"] == "ok" and not any(c["rets"]) and any(st) and (
                (algo == "recursivedoubling" and P & (P - 1))):
            # deviation: the reference returns MPI_SUCCESS without
            # gathering at non-power-of-two P (libbine_allgather.c:31-34)
            if not all(x == 1 for x in st):
                bad.append((c["id"], "status", st))
            continue
        if c["status"] != "ok" or any(c["rets"]):
            # the reference errors (rets), asserts or hangs (no_output): the product
            # returns the mapped status, or -- where the reference crashed on its own
            # heap overflow (static, N=333) -- the correct result
            if c["status"] == "ok":
                exp_st = [STATUS_OF_MPI[x] for x in c["rets"]]
                if st != exp_st:
                    bad.append((c["id"], "status", st, exp_st))
            elif any(st):
                if not all(x == 1 for x in st):
                    bad.append((c["id"], "status", st))
            else:
                # the reference crashed (e.g. MPI_IN_PLACE in the block-by-block
                # and remap variants, which read it as a buffer): vs the oracle
                want = oracle_outputs(coll, algo, sb, dt, c["op"], rk, c["segsize"], root, in_place=ip)
                if coll == "reduce_scatter" and P == 1 and algo in ("butterfly", "bine_block_by_block"):
                    want = [sb[0][: rk[0]]]   # the P = 1 copy the reference omits (DESIGN.md deviations)
                if any(sha(o) != sha(w) for o, w in zip(outs, want)):
                    bad.append((c["id"], "vs-oracle"))
            continue
        if any(st):
            bad.append((c["id"], "status", st))
            continue
        miss = G.check_rank_outputs(c, outs)
        if miss:
            # documented deviations: the segmented tail bug and the P=1 no-ops
            if algo == "bine_bdw_remap_segmented":
                want, _ = O.allreduce(algo, sb, dt, c["op"], c["segsize"], ref_bugs=False)
            elif P == 1 and algo in ("butterfly", "bine_block_by_block"):
                want = [sb[0][: rk[0]]]
            else:
                want = None
            if want is None or any(sha(outs[r]) != sha(want[r]) for r in miss):
                bad.append((c["id"], "ranks", miss))
    assert not bad, bad[:8]


@pytest.mark.parametrize("flat", [0, 1], ids=["literal", "direct"])
@pytest.mark.parametrize("coll", R.ROOTED)
def test_rooted_collectives_large(dev, coll, flat):
    """gather / scatter / alltoall at sizes past the fixtures' (blocks of
    65,537 fp32 and 3 int64 elements, P = 2, 4, 8, two roots) in the literal
    schedule and the direct form (bine_comm_set_flat_ag): bit-exact vs the
    collective (the reference delivers it at these (P, root), rooted_util)"""
    bad = []
    for P in (2, 4, 8):
        for c in comms(P):
            c.set_flat_ag(flat)
        try:
            for dt, n in (("float", 65537), ("int64", 3)):
                for root in ([0] if coll == "alltoall" else [0, P // 2]):
                    sb = R.inputs(coll, dt, n, P, seed_base=77)
                    want, exp = R.expect(coll, sb, dt, root, P, n)
                    assert exp == 0
                    outs, st = run_loopback(coll, "bine", sb, dt, root=root)
                    if any(st) or any(O.canonical(o) != (b"" if w is None else O.canonical(w)) for o, w in zip(outs, want)):
                        bad.append((coll, P, dt, root, st))
        finally:
            for c in comms(P):
                c.set_flat_ag(0)
    assert not bad, bad


@pytest.mark.parametrize("relay", [0, 4096], ids=["direct", "relay"])
@pytest.mark.parametrize("algo", ["bine_bdw_remap", "bine_bdw_static", "bine_bdw_remap_segmented"])
def test_large_allreduce_digest_matches_reference(dev, algo, relay):
    """N = 1,000,003 fp32, P = 8 against the reference's digests (segmented: the
    reference's own output carries its tail bug -> compared with remap's)."""
    seg = 65536 if algo == "bine_bdw_remap_segmented" else 0
    gal = "bine_bdw_remap" if algo == "bine_bdw_remap_segmented" else algo
    c = G.select(coll="allreduce", algo=gal, P=8, N=1000003, dtype="float", segsize=0)[0]
    sb = O.inputs("float", 1000003, 8)
    outs, st = run_loopback("allreduce", algo, sb, "float", segsize=seg, relay=relay)
    assert not any(st)
    assert G.check_rank_outputs(c, outs) == []


@pytest.mark.parametrize("chunk", [64, 4096, 1 << 20])
def test_pipelined_chunks_bit_exact(dev, chunk):
    """The executor's chunked exchange/reduce overlap must not change a bit."""
    P, n = 8, 300007
    sb = O.inputs("float", n, P)
    want, _ = O.allreduce("bine_bdw_remap", sb, "float")
    outs, st = run_loopback("allreduce", "bine_bdw_remap", sb, "float", segsize=chunk)
    assert not any(st)
    assert all(sha(o) == sha(w) for o, w in zip(outs, want))


@pytest.mark.parametrize("chunk", [256, 65536, 4 << 20])
def test_comm_chunk_setting_bit_exact(dev, chunk):
    """bine_comm_set_chunk (the bench's chunk trials) re-cuts every pipelined
    step of every collective; results stay the reference's"""
    P, per = 8, 40009
    rc = [per] * P
    sb = O.inputs("float", per * P, P)
    want_rs, _ = O.reduce_scatter("bine_permute_remap", sb, rc, "float")
    want_ar, _ = O.allreduce("bine_bdw_static", sb, "float")
    try:
        for c in comms(P):
            c.set_chunk(chunk)
        outs, st = run_loopback("reduce_scatter", "bine_permute_remap", sb, "float", rcounts=rc)
        assert not any(st)
        assert all(sha(o) == sha(w) for o, w in zip(outs, want_rs))
        outs, st = run_loopback("allreduce", "bine_bdw_static", sb, "float", relay=4096)
        assert not any(st)
        assert all(sha(o) == sha(w) for o, w in zip(outs, want_ar))
    finally:
        for c in comms(P):
            c.set_chunk(0)
            c.set_relay(0)


@pytest.mark.parametrize("P", [2, 4, 8])
def test_flat_allgather_bit_exact(dev, P):
    """flat allgather phase (one all-peers exchange after the Bine
    reduce-scatter), alone and with the relayed reduce-scatter: the reference's
    bits, in and out of place"""
    bad = []
    try:
        for c in comms(P):
            c.set_flat_ag(True)
        for dt, n in (("float", 100003), ("double", 4099)):  # flat gather of reduce_bine_bdw
            sb = O.inputs(dt, n, P)
            want, _ = O.reduce("bine_bdw", sb, dt)
            outs, st = run_loopback("reduce", "bine_bdw", sb, dt)
            if any(st) or sha(outs[0]) != sha(want):
                bad.append(("reduce_bine_bdw", dt, st))
        for algo in ("bine_bdw_remap", "bine_bdw_static", "bine_bdw_remap_segmented", "rabenseifner"):
            for dt, n in (("float", 100003), ("int64", 4099), ("double", 7)):
                sb = O.inputs(dt, n, P)
                want, _ = O.allreduce(algo, sb, dt, segsize=4096)
                for relay in (0, 4096):
                    for ip in (False, True):
                        outs, st = run_loopback("allreduce", algo, sb, dt, segsize=4096, relay=relay, in_place=ip)
                        if any(st) or any(sha(o) != sha(w) for o, w in zip(outs, want)):
                            bad.append((algo, dt, relay, ip, st))
    finally:
        for c in comms(P):
            c.set_flat_ag(False)
            c.set_relay(0)
    assert not bad, bad[:8]


def _host_tree(leaves, dtype, op):
    """the reduction tree on the host with the oracle's MPI_Reduce_local:
    level by level v[i] = v[i] (op) v[i + w], v[i] = inout"""
    v = [np.array(x).copy() for x in leaves]
    w = 1
    while w < len(v):
        for i in range(0, len(v), 2 * w):
            O.reduce_local(np.ascontiguousarray(v[i + w]), v[i], dtype, op)
        w *= 2
    return v[0]


@pytest.mark.parametrize("nl", [2, 4, 8, 16])
@pytest.mark.parametrize("dtype", ALL_DT)
def test_reduce_tree_kernel_bit_exact(dev, nl, dtype):
    """bine_reduce_tree (the flat reduce-scatter's fused kernel) vs the oracle's
    pairwise MPI_Reduce_local tree: every op, vector body + head/tail, and
    leaves not co-aligned mod 16 B (scalar path)"""
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    for op in ("sum", "prod", "max", "min"):
        for n, shift in ((100003, 0), (4096, 0), (3, 0), (5001, esz if esz < 16 else 0)):
            host = [O.fill(dtype, n, 300 + j) for j in range(nl)]
            want = _host_tree(host, dtype, op)
            leaves = []
            for j, h in enumerate(host):
                t = to_dev(h, pad=16 + shift)
                if shift and j % 2:  # odd leaves one element off the others' 16-B phase
                    t2 = torch.zeros_like(t)
                    t2[shift:shift + h.nbytes] = t[:h.nbytes]
                    t = t2[shift:]
                leaves.append(t)
            out = torch.zeros(n * esz + 64, dtype=torch.uint8, device="cuda:0")
            assert pico_amd.reduce_tree(leaves, out, n, dtype, op) == 0
            torch.cuda.synchronize()
            assert sha(from_dev(out, dtype, n)) == sha(want), (op, n, shift)


@pytest.mark.parametrize("dtype", ["int8", "int16", "float", "double"])
def test_reduce_tree_unaligned_but_coaligned(dev, dtype):
    """every leaf and the output start at the same offset past a 16-B boundary:
    the vector body plus the head / tail edges launch"""
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    for nl in (2, 8, 16):
        for shift in range(1, 16 // esz):
            n = 4099
            host = [O.fill(dtype, n, 700 + j) for j in range(nl)]
            want = _host_tree(host, dtype, "sum")
            leaves = []
            for h in host:
                t = torch.zeros(h.nbytes + 64, dtype=torch.uint8, device="cuda:0")
                t[shift * esz:shift * esz + h.nbytes] = torch.from_numpy(h.view(np.uint8).copy()).to("cuda:0")
                leaves.append(t[shift * esz:])
            out = torch.zeros(n * esz + 64, dtype=torch.uint8, device="cuda:0")
            o = out[shift * esz:]
            assert pico_amd.reduce_tree(leaves, o, n, dtype, "sum") == 0
            torch.cuda.synchronize()
            assert sha(from_dev(out, dtype, n, shift * esz)) == sha(want), (nl, shift)


def test_reduce_tree_special_values(dev):
    """NaN / inf / -0 / denormals keep MPICH's operand-order semantics inside
    the fused tree (the same selects and IEEE adds as the pairwise kernel):
    bit-exact with one NaN encoding (as test_reduce_local_special_values);
    when NaNs of both signs meet in one add the two ISAs may return either
    input NaN, so with mixed-sign NaNs the check is value-level (NaN where
    the host has NaN, bits elsewhere)"""
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 3.4e38, -3.4e38]
    rng = np.random.default_rng(7)
    for mixed in (False, True):
        vals = np.array(specials + ([-np.nan] if mixed else []), np.float32)
        host = [rng.choice(vals, 4099).astype(np.float32) for _ in range(8)]
        for op in ("sum", "prod", "max", "min"):
            want = _host_tree(host, "float", op)
            out = torch.zeros(4099 * 4 + 64, dtype=torch.uint8, device="cuda:0")
            assert pico_amd.reduce_tree([to_dev(h) for h in host], out, 4099, "float", op) == 0
            torch.cuda.synchronize()
            got = from_dev(out, "float", 4099)
            if not mixed:
                assert sha(got) == sha(want), op
            else:
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan), op
                assert got[~nan].tobytes() == want[~nan].tobytes(), op


FLAT_RS = [("allreduce", "bine_bdw_remap"), ("allreduce", "bine_bdw_static"),
           ("allreduce", "bine_bdw_remap_segmented"), ("reduce_scatter", "bine_permute_remap"),
           ("reduce_scatter", "bine_send_remap"), ("reduce_scatter", "bine_static"),
           ("reduce_scatter", "bine_block_by_block"), ("reduce", "bine_bdw"),
           ("allreduce", "rabenseifner"), ("reduce_scatter", "recursivehalving"), ("reduce", "bine_lat"),
           ("allreduce", "bine_lat"), ("allreduce", "recursivedoubling"),
           ("reduce_scatter", "recursive_distance_doubling"), ("reduce_scatter", "butterfly"),
           ("allreduce", "bine_block_by_block_any_even"), ("reduce_scatter", "bine_block_by_block_any_even"),
           ("allreduce", "ring"), ("reduce_scatter", "ring")]


@pytest.mark.parametrize("P", [2, 4, 8])
def test_flat_reduce_scatter_bit_exact(dev, P):
    """flat reduce-scatter phase (one all-peers exchange, one fused tree per
    chunk) on the device: the reference's bits for every algorithm it applies
    to, chunked and not, in and out of place, with the flat allgather too"""
    bad = []
    cs = comms(P)
    try:
        for c in cs:
            c.set_flat_rs(True)
        for coll, algo in FLAT_RS:
            for dt, n in (("float", 100003), ("int64", 4099), ("double", 7)):
                for chunk in (0, 4096):
                    for flat_ag in (False, True):
                        for c in cs:
                            c.set_chunk(chunk)
                            c.set_flat_ag(flat_ag)
                        for ip in (False, True):
                            if coll == "allreduce":
                                sb = O.inputs(dt, n, P)
                                want, _ = O.allreduce(algo, sb, dt, segsize=4096)
                                outs, st = run_loopback(coll, algo, sb, dt, segsize=4096, in_place=ip)
                            elif coll == "reduce_scatter":
                                rc = [n // P + 1] * P if algo == "bine_permute_remap" else \
                                    [n // P + (i % 3) for i in range(P)]
                                sb = O.inputs(dt, sum(rc), P)
                                want, _ = O.reduce_scatter(algo, sb, rc, dt)
                                outs, st = run_loopback(coll, algo, sb, dt, rcounts=rc, in_place=ip)
                            else:
                                sb = O.inputs(dt, n, P)
                                w, _ = O.reduce(algo, sb, dt)
                                outs, st = run_loopback(coll, algo, sb, dt, in_place=ip)
                                want, outs = [w], outs[:1]
                            if any(st) or any(sha(o) != sha(w) for o, w in zip(outs, want)):
                                bad.append((coll, algo, dt, chunk, flat_ag, ip, st))
    finally:
        for c in cs:
            c.set_flat_rs(False)
            c.set_flat_ag(False)
            c.set_chunk(0)
    assert not bad, bad[:8]


@pytest.mark.parametrize("P", [8, 16])
def test_flat_reduce_scatter_ops_and_dtypes(dev, P):
    """flat reduce-scatter + flat allgather for every operator and the narrow
    integer types (the tree kernel's 16-element-per-vector paths), P = 8 and
    P = 16 (16 leaves: two 8-leaf groups), with blocks of 0 and 1 element"""
    bad = []
    cs = comms(P)
    try:
        for c in cs:
            c.set_flat_rs(True)
            c.set_flat_ag(True)
            c.set_chunk(4096)
        for dt in ("int8", "uint16", "int32", "float", "double"):
            for op in ("sum", "prod", "max", "min"):
                for n in (P // 2, 4099):
                    sb = O.inputs(dt, n, P)
                    want, _ = O.allreduce("bine_bdw_remap", sb, dt, op=op)
                    outs, st = run_loopback("allreduce", "bine_bdw_remap", sb, dt, op=op)
                    if any(st) or any(sha(o) != sha(w) for o, w in zip(outs, want)):
                        bad.append(("allreduce", dt, op, n, st))
                rc = [3 + (i % 2) for i in range(P)]
                sb = O.inputs(dt, sum(rc), P)
                want, _ = O.reduce_scatter("bine_static", sb, rc, dt, op=op)
                outs, st = run_loopback("reduce_scatter", "bine_static", sb, dt, op=op, rcounts=rc)
                if any(st) or any(sha(o) != sha(w) for o, w in zip(outs, want)):
                    bad.append(("rs_static", dt, op, st))
    finally:
        for c in cs:
            c.set_flat_rs(False)
            c.set_flat_ag(False)
            c.set_chunk(0)
    assert not bad, bad[:8]


def test_flat_block_by_block_swapped_level_on_device(dev):
    """the tree kernel's swapped top level (block_by_block's last step reduces
    (own, received)) with signed zeros and NaNs under MAX / MIN: the
    reference's bits"""
    P = 8
    rng = np.random.default_rng(3)
    vals = np.array([0.0, -0.0, np.nan, 1.0, -1.0], np.float32)
    rc = [4099 + (i % 2) for i in range(P)]
    sb = [rng.choice(vals, sum(rc)).astype(np.float32) for _ in range(P)]
    cs = comms(P)
    try:
        for c in cs:
            c.set_flat_rs(True)
        for op in ("max", "min", "sum"):
            want, _ = O.reduce_scatter("bine_block_by_block", sb, rc, "float", op=op)
            outs, st = run_loopback("reduce_scatter", "bine_block_by_block", sb, "float", op=op, rcounts=rc)
            assert not any(st)
            if op == "sum":  # NaN payloads of mixed-sign NaN sums: value-level (see test_reduce_tree_special_values)
                assert all(np.array_equal(np.isnan(o), np.isnan(w)) for o, w in zip(outs, want))
            else:
                assert all(o.tobytes() == w.tobytes() for o, w in zip(outs, want)), op
    finally:
        for c in cs:
            c.set_flat_rs(False)


def test_per_op_profile(dev):
    """bine_comm_set_profile: one timed entry per op of the issue schedule
    (exchanges with their send bytes, local ops with algorithmic HBM bytes),
    starts ordered within each stream; results unchanged"""
    P, n = 4, 1 << 20
    cs = comms(P)
    sb = O.inputs("float", n, P)
    want, _ = O.allreduce("bine_bdw_remap", sb, "float")
    try:
        for c in cs:
            c.set_profile(True)
            c.set_flat_rs(True)
            c.set_flat_ag(True)
            c.set_chunk(1 << 20)
        outs, st = run_loopback("allreduce", "bine_bdw_remap", sb, "float")
        assert not any(st) and all(sha(o) == sha(w) for o, w in zip(outs, want))
        for r, c in enumerate(cs):
            ops = c.profile()
            sched, _, _ = pico_amd.schedule("allreduce", "bine_bdw_remap", P, r, count=n, esz=4, chunk_bytes=1 << 20,
                                            flat_rs=True, flat_ag=True)
            assert len(ops) == len(sched)
            for o, s in zip(ops, sched):
                assert o["xchg"] == s["xchg"] and o["nprims"] == len(s["prims"]) and o["ms"] >= 0
                if s["xchg"]:
                    assert o["bytes"] == 4 * sum(p["count"] for p in s["prims"] if p["type"] == "SEND")
                else:
                    assert o["bytes"] == sum((p["peer"] + 1) * p["count"] * 4 for p in s["prims"])
            for kind in (0, 1):
                starts = [o["start_ms"] for o in ops if o["xchg"] == kind]
                assert starts == sorted(starts)
    finally:
        for c in cs:
            c.set_profile(False)
            c.set_flat_rs(False)
            c.set_flat_ag(False)
            c.set_chunk(0)


@pytest.mark.parametrize("algo", list(pico_amd.ALGOS["allreduce"]))
def test_in_place_allreduce(dev, algo):
    P = 4
    sb = O.inputs("double", 1001, P)
    want, _ = O.allreduce(algo, sb, "double", segsize=64)
    outs, st = run_loopback("allreduce", algo, sb, "double", segsize=64, in_place=True)
    assert not any(st)
    assert all(sha(o) == sha(w) for o, w in zip(outs, want))


def test_large_reduce_scatter_checksum(dev):
    """C4 shape scaled to one GPU: permute_remap RS, P = 8, 4 Mi elements per
    rank-block; checksum of each rank's block against the oracle's."""
    P, per = 8, 1 << 19
    rc = [per] * P
    sb = O.inputs("float", per * P, P)
    want, _ = O.reduce_scatter("bine_permute_remap", sb, rc, "float")
    for relay in (0, 65536):
        outs, st = run_loopback("reduce_scatter", "bine_permute_remap", sb, "float", rcounts=rc, relay=relay)
        assert not any(st)
        assert [host_checksum(o) for o in outs] == [host_checksum(w) for w in want]


# ---- RCCL transport (single rank on this box) --------------------------------------

def test_rccl_single_rank(dev):
    uid = pico_amd.Comm.unique_id()
    c = pico_amd.Comm.rccl(0, 1, uid, 0)
    try:
        a = O.fill("float", 4097, 3)
        ta = to_dev(a)
        tr = torch.zeros_like(ta)
        pico_amd.allreduce_bine_bdw_remap(ta, tr, a.size, "float", "sum", c)
        c.synchronize()
        torch.cuda.synchronize()
        assert from_dev(tr, "float", a.size).tobytes() == a.tobytes()
        with pytest.raises(pico_amd.BineError) as ei:
            pico_amd.allreduce_bine_bdw_static(ta, tr, a.size, "float", "sum", c)   # reference: MPI_ERR_ARG at P=1
        assert ei.value.status == 1
    finally:
        c.destroy()


def test_unordered_fill_of_the_round4_harness_races(dev):
    """DESIGN.md 7.1, candidate (i): the round-4 form of
    tools/rccl_large.py filled the collective's input with fill_pico on
    torch's default stream (the legacy NULL stream) and issued the collective
    inside `with torch.cuda.stream(side)` -- a torch pool stream, created
    non-blocking, so nothing ordered the two.  Here the NULL stream is held
    busy first (torch.cuda._sleep), which makes the race certain instead of
    rare: in the round-4 form the collective (P = 1: the copy sbuf -> rbuf)
    reads the input before the fill and the output's digest is wrong; with
    the ordering the harness has now (torch.cuda.synchronize() between fill
    and collective) it is right.  The race can touch only the FIRST call
    after a fill -- every later call of that harness came after a
    device-wide synchronize -- so it cannot be the round-4 failure of all 16
    calls.  The side stream is a high-priority one: HIP keeps
    a separate HW queue pool per priority, so it cannot share a hardware
    queue with the NULL stream -- which, with the suite's few queues per
    process (tests/conftest.py), would order the two by accident and hide
    the race."""
    n = 1 << 24   # 64 MiB fp32
    want = pico_amd.checksum(_filled(n), n, "float")
    uid = pico_amd.Comm.unique_id()
    c = pico_amd.Comm.rccl(0, 1, uid, 0)
    side = torch.cuda.Stream(priority=-1)
    s = torch.zeros(n, dtype=torch.float32, device=dev)
    r = torch.zeros(n, dtype=torch.float32, device=dev)
    try:
        def run(ordered):
            s.zero_()
            r.fill_(float("nan"))
            with torch.cuda.stream(side):   # warm: plans and workspace exist, nothing implicit syncs
                pico_amd.allreduce("bine_bdw_remap", s, r, n, "float", "sum", c)
            torch.cuda.synchronize()
            c.synchronize()
            torch.cuda._sleep(200_000_000)                 # the NULL stream busy for ~0.1 s
            pico_amd.fill_pico(s, n, "float", 1234)       # on the NULL stream, after the sleep
            if ordered:
                torch.cuda.synchronize()
            with torch.cuda.stream(side):
                pico_amd.allreduce("bine_bdw_remap", s, r, n, "float", "sum", c)
            torch.cuda.synchronize()
            c.synchronize()
            return pico_amd.checksum(r, n, "float") == want
        assert run(ordered=False) is False   # the round-4 form reads the input before its fill
        assert run(ordered=True) is True
    finally:
        c.destroy()


def _filled(n):
    t = torch.empty(n, dtype=torch.float32, device="cuda:0")
    pico_amd.fill_pico(t, n, "float", 1234)
    torch.cuda.synchronize()
    return t


# ---- pico_core-compatible device-resident driver ----------

@pytest.mark.parametrize("coll,algo,dtype", [("ALLREDUCE", "bine_bdw_remap_over", "float"),
                                             ("REDUCE_SCATTER", "bine_permute_remap_over", "int64"),
                                             ("ALLGATHER", "k_bruck_over", "double"),
                                             ("REDUCE", "bine_bdw_over", "int32"),
                                             ("BCAST", "bine_lat_over", "float"),
                                             ("GATHER", "bine_over", "int32"),
                                             ("SCATTER", "bine_over", "double"),
                                             ("ALLTOALL", "bine_over", "int64")])
def test_pico_amd_core_writes_pico_core_csv(dev, tmp_path, coll, algo, dtype):
    """pico_amd_core: pico_core's CLI / env / ground-truth check / CSV layout,
    buffers in HBM, calls through libbine.so's libbine.h symbols.  One rank
    (the Bine allgathers return MPI_ERR_ARG at P = 1, like the reference)."""
    exe = os.path.join(ROOT, "pico_amd", "lib", "pico_amd_core")
    env = dict(os.environ, COLLECTIVE_TYPE=coll, OUTPUT_DIR=str(tmp_path), DATA_DIR=str(tmp_path),
               OUTPUT_LEVEL="all", LOCATION="local", SEGMENTED="no", PICO_SEED="1234",
               PATH="/opt/conda/bin:" + os.environ.get("PATH", ""))
    p = _sub.run_kw(["/opt/conda/bin/mpiexec", "-n", "1", exe, "1048576", "5", algo, dtype], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    csv = tmp_path / f"1048576_{algo}_{dtype}.csv"
    lines = csv.read_text().splitlines()
    assert lines[0] == "highest,rank0" and len(lines) == 6
    assert all(int(x.split(",")[0]) > 0 for x in lines[1:])
    assert (tmp_path / "alloc_1_GPU.csv").read_text().startswith("MPI_Rank,allocation\n0,")


@pytest.mark.parametrize("coll,algo,dtype", [("BCAST", "bine_bdw_remap_over", "float"),
                                             ("GATHER", "bine_over", "int64"), ("SCATTER", "bine_over", "float"),
                                             ("ALLTOALL", "bine_over", "int8"), ("ALLREDUCE", "bine_bdw_remap_over", "int32")])
def test_pico_amd_core_two_ranks(dev, tmp_path, coll, algo, dtype):
    """pico_amd_core with 2 ranks sharing the GPU (distinct RCCL host ids):
    every rank's result checked against MPICH's PMPI_* collective, as
    pico_core does, for the round-5 collectives"""
    exe = os.path.join(ROOT, "pico_amd", "lib", "pico_amd_core")
    env = dict(os.environ, COLLECTIVE_TYPE=coll, OUTPUT_DIR=str(tmp_path), DATA_DIR=str(tmp_path),
               OUTPUT_LEVEL="summarized", LOCATION="local", SEGMENTED="no", PICO_SEED="99", BINE_FAKE_HOSTS="1",
               PATH="/opt/conda/bin:" + os.environ.get("PATH", ""))
    cmd = ["/opt/conda/bin/mpiexec"]
    for r in range(2):   # one RCCL host id per rank: two ranks on ONE GPU (integration/run_pico_core.sh)
        cmd += ([":"] if r else []) + ["-n", "1", "-env", "NCCL_HOSTID", f"fake-host-{r}", "-env",
                                       "NCCL_SOCKET_IFNAME", "lo", exe, "1048576", "4", algo, dtype]
    p = _sub.run_kw(cmd, env=env, capture_output=True, text=True, timeout=150, ranks=2)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Last Iter Time" in p.stdout
    assert len((tmp_path / f"1048576_{algo}_{dtype}.csv").read_text().splitlines()) == 5


PICO_CORE = os.path.join(ROOT, "integration", "_build", "pico_core")


# libbine.so's forms (bine_dropin_defaults): "default" = no
# BINE_* setting at all (the flat phases over the direct transport, the whole
# call as one k_dm_fused launch where its plan fits); "literal" = BINE_LITERAL=1
# (the reference's literal schedule over RCCL P2P); "rccl" = BINE_DIRECT=0 (the
# flat phases over RCCL P2P).  BINE_FAKE_HOSTS is the harness's (two ranks on
# one GPU need distinct RCCL host ids, integration/run_pico_core.sh).
FORMS = {"default": {}, "literal": {"BINE_LITERAL": "1"}, "rccl": {"BINE_DIRECT": "0"},
         # the default forms with small host buffers staged through device
         # buffers instead of addressed in place (zero copy)
         "staged": {"BINE_HOST_ZERO_COPY_BYTES": "0"}}


@pytest.mark.skipif(not os.path.exists(PICO_CORE), reason="reference pico_core not built (integration/Makefile)")
@pytest.mark.parametrize("np_,coll,algo,dtype,form,count", [
    (1, "ALLREDUCE", "bine_bdw_remap_over", "float", "default", "1048576"),
    # staged in pipelined chunks (libbine.so with_buffers): P = 1 is a copy, int64
    # SUM is exact in any association -- both cut the buffer into 16 MiB chunks
    (1, "ALLREDUCE", "bine_bdw_remap_over", "float", "default", "67108864"),
    (2, "ALLREDUCE", "bine_bdw_remap_over", "int64", "default", "8388608"),
    (2, "ALLREDUCE", "bine_bdw_remap_over", "float", "literal", "16777216"),
    # floating point at P > 1: the staging pipelined into the collective
    # (bine_allreduce_staged / bine_reduce_scatter_staged), over the direct
    # peer-memory transport (the default) and over RCCL
    (4, "ALLREDUCE", "bine_bdw_remap_over", "float", "default", "16777216"),
    (4, "ALLREDUCE", "bine_bdw_static_over", "double", "default", "8388608"),
    (4, "ALLREDUCE", "bine_bdw_remap_over", "float", "literal", "16777216"),
    (2, "REDUCE_SCATTER", "bine_permute_remap_over", "float", "literal", "16777216"),
    (2, "REDUCE_SCATTER", "bine_permute_remap_over", "float", "default", "16777216"),
    (2, "ALLREDUCE", "bine_bdw_remap_over", "float", "rccl", "1048576"),
    (2, "ALLREDUCE", "bine_lat_over", "double", "default", "1048576"),
    (2, "REDUCE_SCATTER", "bine_permute_remap_over", "int64", "default", "1048576"),
    (2, "REDUCE", "bine_bdw_over", "float", "literal", "1048576"),
    (2, "REDUCE", "bine_bdw_over", "float", "default", "1048576"),
    (2, "BCAST", "bine_lat_over", "float", "default", "1048576"),
    (2, "BCAST", "bine_lat_new_over", "int64", "literal", "1048576"),
    (2, "GATHER", "bine_over", "float", "default", "1048576"),
    (2, "SCATTER", "bine_over", "int64", "default", "1048576"),
    (2, "ALLTOALL", "bine_over", "float", "rccl", "1048576"),
])
def test_reference_pico_core_dropin(dev, tmp_path, np_, coll, algo, dtype, form, count):
    """the reference's UNCHANGED pico_core (integration/Makefile links it against
    libbine.so) drives the GPU path through the libbine.h symbols and checks
    every result against MPICH's own PMPI_* collective (pico_core_utils.c:
    553-610), aborting on a mismatch; 2 ranks share the GPU through RCCL's
    socket transport (distinct NCCL_HOSTIDs), in libbine.so's default forms,
    the literal schedule, or the flat phases over RCCL"""
    env = dict(os.environ, PICO_OUT=str(tmp_path), BINE_FAKE_HOSTS="1", **FORMS[form])
    p = _sub.run_kw(["bash", os.path.join(ROOT, "integration", "run_pico_core.sh"), str(np_), coll, count,
                        "5", algo, dtype], env=env, capture_output=True, text=True, timeout=150, ranks=np_)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    assert "Last Iter Time" in p.stdout


@pytest.mark.skipif(not os.path.exists(PICO_CORE), reason="reference pico_core not built (integration/Makefile)")
@pytest.mark.parametrize("algo,form", [("bine_bdw_remap_over", "default"), ("bine_bdw_remap_over", "literal"),
                                       ("bine_bdw_remap_over", "rccl"), ("bine_lat_over", "default"),
                                       ("bine_bdw_remap_over", "staged")])
def test_reference_pico_core_c1(dev, tmp_path, algo, form):
    """BASELINE configs[0] (C1) through the GPU path exactly as the reference
    runs it: the unchanged pico_core, 4 ranks, 262,144 fp32 elements (1 MiB)
    per rank, allreduce SUM (pico_core_utils.h:262), 20 iterations, every one
    checked by pico_core against MPICH's PMPI_Allreduce (pico_core_utils.c:
    553-610, 960-992); the 4 ranks share the GPU through RCCL's socket
    transport (distinct NCCL_HOSTIDs); host buffers.  "default": no BINE_*
    setting -- libbine.so's own choice (the flat phases over
    the direct transport, one k_dm_fused launch, the host buffers addressed in
    place); "staged": the same through device buffers"""
    env = dict(os.environ, PICO_OUT=str(tmp_path), BINE_FAKE_HOSTS="1", **FORMS[form])
    for k in ("BINE_LITERAL", "BINE_DIRECT", "BINE_FLAT_RS", "BINE_FLAT_AG"):
        if k not in FORMS[form]:
            env.pop(k, None)
    p = _sub.run_kw(["bash", os.path.join(ROOT, "integration", "run_pico_core.sh"), "4", "ALLREDUCE", "262144",
                        "20", algo, "float"], env=env, capture_output=True, text=True, timeout=150, ranks=4)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    assert "Last Iter Time" in p.stdout
    csv = tmp_path / "data" / f"262144_{algo}_float.csv"
    lines = csv.read_text().splitlines()
    assert lines[0].startswith("highest,rank0,rank1,rank2,rank3") and len(lines) == 21


OP_CHECK = os.path.join(ROOT, "integration", "_build", "op_check")


@pytest.mark.skipif(not os.path.exists(OP_CHECK), reason="integration/op_check not built (integration/Makefile)")
@pytest.mark.parametrize("np_,form", [(1, "default"), (2, "literal"), (2, "default"), (2, "rccl"), (2, "staged")])
def test_mpi_typed_entry_points_match_mpich(dev, np_, form):
    """integration/op_check: libbine.so's MPI-typed entry points (allreduce,
    reduce_scatter, reduce, bcast, allgather, gather, scatter, alltoall; host
    buffers) equal MPICH's own PMPI_* collectives
    for every order-independent (type, op) pair, and return MPI_ERR_OP where
    MPICH rejects the pair; 2 ranks share the GPU as above"""
    env = dict(os.environ, BINE_FAKE_HOSTS="1", **FORMS[form])
    p = _sub.run_kw(["bash", os.path.join(ROOT, "integration", "run_op_check.sh"), str(np_)], env=env,
                       capture_output=True, text=True, timeout=150, ranks=np_)
    assert p.returncode == 0 and "OPCHECK ok" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])


CHURN = os.path.join(ROOT, "integration", "_build", "buffer_churn")


@pytest.mark.skipif(not os.path.exists(CHURN), reason="integration/buffer_churn not built (integration/Makefile)")
@pytest.mark.parametrize("np_", [1, 2])
def test_libbine_host_buffers_freed_and_reallocated(dev, np_):
    """integration/buffer_churn: libbine.so's
    allreduce_bine_bdw_remap on 64 MiB malloc buffers, the buffers freed and
    malloc'd again at the same addresses, new data, a second call -- both vs
    PMPI_Allreduce, in and out of place, float and int64, and no caller buffer
    left page-locked after a call; at P = 2 also rank 0's buffers on the
    device and rank 1's on the host in one call (allreduce and
    reduce_scatter, below and above the staging pipeline's threshold)"""
    env = dict(os.environ, BINE_FAKE_HOSTS="1", BINE_SYNC_TIMEOUT_S="60")
    p = _sub.run_kw(["bash", os.path.join(ROOT, "integration", "run_op_check.sh"), str(np_), "buffer_churn"],
                       env=env, capture_output=True, text=True, timeout=150, ranks=np_)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "CHURN ok" in p.stdout, (p.stdout[-2000:], p.stderr[-1500:])
    assert "same addresses: yes" in p.stdout  # glibc mmap reuse: the hazard's shape was exercised


DM_TIMEOUT = os.path.join(ROOT, "integration", "_build", "dm_timeout")


@pytest.mark.skipif(not os.path.exists(DM_TIMEOUT), reason="integration/dm_timeout not built (integration/Makefile)")
def test_libbine_timed_out_call_returns_an_error(dev):
    """integration/dm_timeout: through libbine.so with the
    direct transport (BINE_DIRECT=1) and a wait limit that every wait exceeds
    (BINE_DIRECT_TIMEOUT_S=1e-7), the call in which a wait timed out returns
    an MPI error itself -- never MPI_SUCCESS with a wrong rbuf -- and so does
    the next one; 2 ranks share the GPU"""
    env = dict(os.environ, BINE_FAKE_HOSTS="1", BINE_DIRECT="1", BINE_DIRECT_TIMEOUT_S="1e-7",
               BINE_SYNC_TIMEOUT_S="60")
    p = _sub.run_kw(["bash", os.path.join(ROOT, "integration", "run_op_check.sh"), "2", "dm_timeout"],
                    env=env, capture_output=True, text=True, timeout=150, ranks=2)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "DMTIMEOUT ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    assert "RESULT WRONG" not in p.stdout
    assert "waited" in p.stderr   # the error carries the timed-out waiter's record


@pytest.mark.parametrize("relay", [0, 64, "flat"], ids=["direct", "relay", "flat"])
@pytest.mark.parametrize("P", [2, 4, 6, 8])
def test_allgather_family_matches_oracle(dev, P, relay):
    """all 12 allgather algorithms, device path vs the oracle's restatement of
    the reference (golden-pinned on the CPU side), incl. 1-byte elements;
    "flat": every algorithm as one all-peers exchange"""
    bad = []
    flat = relay == "flat"
    relay = 0 if flat else relay
    for c in comms(P):
        c.set_flat_ag(flat)
    for algo in pico_amd.ALGOS["allgather"]:
        for dt, n in (("float", 1), ("int8", 333), ("double", 4099)):
            sb = O.inputs(dt, n, P)
            want, rets = O.allgather(algo, sb, dt)
            outs, st = run_loopback("allgather", algo, sb, dt, relay=relay)
            if any(rets) or (algo == "recursivedoubling" and P & (P - 1)):
                if not any(st):
                    bad.append((algo, dt, n, "expected an error", rets))
                continue
            if any(st):
                bad.append((algo, dt, n, "status", st))
            elif any(sha(o) != sha(w) for o, w in zip(outs, want)):
                bad.append((algo, dt, n, "data"))
    for c in comms(P):
        c.set_flat_ag(False)
    assert not bad, bad[:8]


# ---- multi-tree mode ------------------------------------------------------------

@pytest.mark.parametrize("P", [4, 8])
def test_multi_tree_allreduce_on_device(dev, P):
    """tree mode on the device: bit-exact vs the relabelled oracle for fp32 /
    fp64, and vs the reference's golden vectors for integers"""
    import test_trees as TT
    bad = []
    try:
        for c in comms(P):
            c.set_trees(True)
        for algo in ("bine_bdw_remap", "bine_bdw_static", "ring", "bine_lat"):
            for dt, n in (("float", 100003), ("double", 4099), ("int32", 65537)):
                sb = O.inputs(dt, n, P)
                want = TT.relabelled_oracle(algo, sb, dt)
                outs, st = run_loopback("allreduce", algo, sb, dt)
                if any(st) or any(sha(o) != sha(w) for o, w in zip(outs, want)):
                    bad.append((algo, dt, n, st))
        for c in G.select(coll="allreduce", algo="bine_bdw_remap", P=P, op="sum"):
            if c["dtype"] not in ("int32", "int64", "int8", "int16", "uint8") or c["status"] != "ok":
                continue
            sb = G.inputs(c)
            outs, st = run_loopback("allreduce", "bine_bdw_remap", sb, c["dtype"])
            if any(st) or G.check_rank_outputs(c, outs):
                bad.append((c["id"], st))
    finally:
        for c in comms(P):
            c.set_trees(False)
    assert not bad, bad[:8]


@pytest.mark.parametrize("P", [4, 8])
def test_multi_tree_reduce_scatter_on_device(dev, P):
    import test_trees as TT
    rc = [(1 << 15) + 3] * P
    try:
        for c in comms(P):
            c.set_trees(True)
        for dt in ("float", "int64"):
            sb = O.inputs(dt, sum(rc), P)
            want = TT.relabelled_rs_oracle(sb, rc, dt)
            outs, st = run_loopback("reduce_scatter", "bine_permute_remap", sb, dt, rcounts=rc)
            assert not any(st)
            assert all(sha(o) == sha(w) for o, w in zip(outs, want)), dt
    finally:
        for c in comms(P):
            c.set_trees(False)


@pytest.mark.parametrize("dtype", ["float", "double", "int8", "int64"])
def test_reduce_batch_matches_per_window(dev, dtype):
    """batched launch (multi-tree rounds): windows of different sizes and 16-B
    phases, heads and tails, vs the oracle's MPI_Reduce_local per window"""
    npdt = O.NP_DTYPES[dtype]
    esz = np.dtype(npdt).itemsize
    sizes = [1, 7, 4097, 100003, 65536, 3, 12345, 1 << 18][: 8]
    ins, ios, host_in, host_io = [], [], [], []
    for k, n in enumerate(sizes):
        a = O.fill(dtype, n, 100 + k)
        b = O.fill(dtype, n, 200 + k)
        shift = (k * esz) % 16  # same phase for both operands of a window

        def placed(x):
            raw = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy())
            t = torch.zeros(raw.numel() + shift + 16, dtype=torch.uint8, device="cuda:0")
            t[shift:shift + raw.numel()] = raw.to("cuda:0")
            return t[shift:]
        ins.append(placed(a))
        ios.append(placed(b))
        host_in.append(a)
        host_io.append(b.copy())
    assert pico_amd.reduce_batch(ins, ios, sizes, dtype) == 0
    torch.cuda.synchronize()
    for k, n in enumerate(sizes):
        O.reduce_local(host_in[k], host_io[k], dtype)
        assert sha(from_dev(ios[k], dtype, n)) == sha(host_io[k]), k
    # not co-aligned -> ERR_ARG (the executor then launches window by window)
    a = to_dev(O.fill(dtype, 64, 1), pad=16)
    b = to_dev(O.fill(dtype, 64, 2), pad=16)
    if esz < 16:
        assert pico_amd.reduce_batch([a[esz:], a], [b, b], [32, 32], dtype) == 1


@pytest.mark.parametrize("P", [4, 8])
def test_known_answer_debug_inputs(dev, P):
    """pico_core's DEBUG known-answer mode (pico_core.c:82-95,
    debug_sbuf_generator pico_core_utils.c:1095-1126): rank r sends 10^r in
    every element, so every allreduce element is sum(10^r) -- for every
    allreduce algorithm, every transport, int32 and int64"""
    n = 10007
    bad = []
    for dt, npdt in (("int32", np.int32), ("int64", np.int64)):
        sb = [np.full(n, 10 ** r, npdt) for r in range(P)]
        want = np.full(n, sum(10 ** r for r in range(P)), npdt)
        for algo in pico_amd.ALGOS["allreduce"]:
            for mode in ("direct", "relay", "flat", "trees"):
                try:
                    for c in comms(P):
                        c.set_trees(mode == "trees")
                        c.set_flat_ag(mode == "flat")
                    outs, st = run_loopback("allreduce", algo, sb, dt, segsize=256,
                                            relay=64 if mode == "relay" else 0)
                finally:
                    for c in comms(P):
                        c.set_trees(False)
                        c.set_flat_ag(False)
                if any(st) or any(not np.array_equal(o, want) for o in outs):
                    bad.append((dt, algo, mode, st))
    assert not bad, bad[:8]


@pytest.mark.parametrize("P", [4, 8])
def test_trees_within_pico_core_tolerance(dev, P):
    """multi-tree mode changes the fp association order: its results must stay
    within pico_core's ground-truth tolerance against an exact (fp64) sum --
    P * 1e-4 absolute for float, P * 1e-13 for double (pico_core_utils.c:967-988)"""
    n = 65537
    try:
        for c in comms(P):
            c.set_trees(True)
        for dt, tol in (("float", P * 1e-4), ("double", P * 1e-13)):
            sb = O.inputs(dt, n, P)
            exact = np.sum(np.stack([x.astype(np.float64) for x in sb]), axis=0)
            outs, st = run_loopback("allreduce", "bine_bdw_remap", sb, dt)
            assert not any(st)
            for o in outs:
                assert np.max(np.abs(o.astype(np.float64) - exact)) <= tol, dt
    finally:
        for c in comms(P):
            c.set_trees(False)


def test_vendor_allreduce_needs_rccl():
    """bine_vendor_allreduce is RCCL's own collective (the bench's baseline):
    on an in-process loopback communicator it reports BINE_ERR_UNSUPPORTED
    (no silent fallback).  Its results over real RCCL are checked in
    tools/rccl_matrix.py (int64 SUM, 4 processes)."""
    c = comms(2)[0]
    x = torch.ones(16, dtype=torch.float32, device="cuda:0")
    with pytest.raises(pico_amd.BineError) as e:
        pico_amd.vendor_allreduce(x, x, 16, "float", "sum", c)
    assert e.value.status == 6  # BINE_ERR_UNSUPPORTED


def test_direct_transport_launch_caps(dev):
    """the residency cap of every direct-transport kernel on this device
    (bine_dm_launch_cap: CUs x (resident blocks per CU - 1) / share):
    k_dm_move's 32 VGPRs hold 8 workgroups per CU, k_dm_move_tree<float, SUM,
    8>'s 96 hold 5 -- 1792 and 1024 slots on MI355X's 256 CUs with one block
    per CU left free; every launch is cut to its cap / ranks on the GPU
    (tests/test_direct_protocol.py)"""
    L = pico_amd.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    mv = L.bine_dm_launch_cap(0, 0, 0, 0, 1)
    tr8 = L.bine_dm_launch_cap(1, pico_amd.DTYPES["float"], pico_amd.OPS["sum"], 8, 1)
    fu = L.bine_dm_launch_cap(2, pico_amd.DTYPES["float"], pico_amd.OPS["sum"], 0, 1)
    print(f"CUs {cus}: k_dm_move {mv}, k_dm_move_tree<f,SUM,8> {tr8}, k_dm_fused<f,SUM> {fu}")
    assert mv > 0 and tr8 > 0 and fu > 0
    assert mv % cus == 0 and tr8 % cus == 0 and fu % cus == 0
    assert mv >= tr8                     # the tree's registers cost residency
    assert L.bine_dm_launch_cap(0, 0, 0, 0, 8) == mv // 8
    props = torch.cuda.get_device_properties(0)
    if props.multi_processor_count == 256 and "gfx950" in props.gcnArchName:
        assert (mv, tr8, fu) == (1792, 1024, 1024)
    assert L.bine_dm_launch_cap(1, pico_amd.DTYPES["float"], pico_amd.OPS["sum"], 3, 1) == -1
