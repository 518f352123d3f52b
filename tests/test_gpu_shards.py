"""Sharded multi-buffer forms on the GPU: the sharded copy (bine_copy_shards /
k_copy_shards) against the host, and bine_reduce_scatter_multi /
bine_allgather_multi over loopback ranks on one GPU -- the reduce-scatter bit
for bit against the existing single call (loopback_reduce_scatter /
loopback_reduce_scatter_wide: not new code) on the rank-major buffer packed on
the host, and for float SUM against the oracle; the allgather against plain
concatenation.  (Graph mode needs an RCCL communicator: tools/shard_check.py,
tests/test_gpu_shards_rccl.py.)"""
import numpy as np
import pytest

import h16_util as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402

TILE = 32 << 10
SIZES = [0, 1, 15, 16, 17, 4095, TILE - 1, TILE, TILE + 1, 3 * TILE + 21]
S = _lib.COPY_SEGS_PER_LAUNCH
RANKS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- bine_copy_shards ----------------------------------------------------------------------

class ShardTable:
    """tensors (flat phase, shard bytes, null) of P shards each in a flat arena
    (every tensor with at least 16 guard bytes before and after it) and their
    packed image, P blocks, in a packed arena (16 guard bytes or more around
    it); the two arenas hold different patterns.  dir 0 copies flat -> packed."""

    def __init__(self, tensors, P, packed_phase, dir):
        self.tensors, self.P, self.dir = tensors, P, dir
        self.foff, f = [], 0
        for fp, nb, _ in tensors:
            self.foff.append(f + 16 + fp)
            f = (f + 16 + fp + P * nb + 16 + 15) & ~15
        self.block = sum(nb for _, nb, _ in tensors)
        self.poff0 = 16 + packed_phase
        psize = (self.poff0 + P * self.block + 16 + 15) & ~15
        a = ((np.arange(max(f + 16, psize), dtype=np.uint64) * 7 + 3) % 251).astype(np.uint8)
        b = ((np.arange(max(f + 16, psize), dtype=np.uint64) * 13 + 5) % 241 + 1).astype(np.uint8) | np.uint8(0x80)
        flat_host, packed_host = (a[:f + 16], b[:psize]) if dir == 0 else (b[:f + 16], a[:psize])
        self.flat_host, self.packed_host = flat_host.copy(), packed_host.copy()
        self.flat = torch.from_numpy(self.flat_host.copy()).to("cuda:0")
        self.packed = torch.from_numpy(self.packed_host.copy()).to("cuda:0")
        assert self.flat.data_ptr() % 16 == 0 and self.packed.data_ptr() % 16 == 0
        self.want_flat, self.want_packed = self.flat_host.copy(), self.packed_host.copy()
        off = 0
        for (fp, nb, _), fo in zip(tensors, self.foff):
            for j in range(P):
                pk = self.poff0 + j * self.block + off
                if dir == 0:
                    self.want_packed[pk:pk + nb] = self.flat_host[fo + j * nb:fo + (j + 1) * nb]
                else:
                    self.want_flat[fo + j * nb:fo + (j + 1) * nb] = self.packed_host[pk:pk + nb]
            off += nb

    def args(self):
        flat = [None if null else self.flat.data_ptr() + fo for (_, _, null), fo in zip(self.tensors, self.foff)]
        return self.packed.data_ptr() + self.poff0, flat, [nb for _, nb, _ in self.tensors], self.P, self.dir

    def check(self):
        for name, got, want in (("flat", self.flat, self.want_flat), ("packed", self.packed, self.want_packed)):
            bad = np.flatnonzero(got.cpu().numpy() != want)      # the copied bytes, the guards, the source
            assert bad.size == 0, f"{name} side: {bad.size} bytes differ, first at {bad[:4]}"


def mixed_tensors(seed):
    """every size twice at random flat phases, zero-length tensors in between
    (some with NULL pointers); the odd sizes make the packed phase, and the
    destination's, differ from shard to shard"""
    rng = np.random.default_rng(seed)
    ts = []
    for rep in range(2):
        for nb in SIZES:
            ts.append((int(rng.integers(0, 16)), nb, nb == 0 and rep == 1))
        ts.append((0, 0, True))
    return ts, int(rng.integers(0, 16))


@pytest.mark.parametrize("dir", [0, 1])
@pytest.mark.parametrize("P", RANKS)
def test_copy_shards_against_host(dev, P, dir):
    ts, pp = mixed_tensors(10 * P + dir)
    t = ShardTable(ts, P, pp, dir)
    pico_amd.copy_shards(*t.args())
    torch.cuda.synchronize()
    t.check()


@pytest.mark.parametrize("dir", [0, 1])
def test_copy_shards_phase_per_shard(dev, dir):
    """co-aligned bases, odd shard sizes: the shift between source and destination
    changes with the shard index -- and 16 tensors whose flat phases run 0..15"""
    t = ShardTable([(0, 2 * TILE + 5, False), (0, 4095, False), (0, 17, False)] +
                   [(fp, TILE + 1, False) for fp in range(16)], 3, 0, dir)
    pico_amd.copy_shards(*t.args())
    torch.cuda.synchronize()
    t.check()


def test_copy_shards_more_than_one_launch(dev):
    """2 * 128 + 37 non-empty tensors with empties in between: three launches"""
    rng = np.random.default_rng(2)
    ts = []
    for k in range(2 * S + 37):
        ts.append((int(rng.integers(0, 16)), int(rng.choice([1, 15, 16, 17, 100, 4095])), False))
        if k % 5 == 0:
            ts.append((0, 0, k % 10 == 0))
    for dir in (0, 1):
        t = ShardTable(ts, 3, 5, dir)
        packed, flat, nb, P, _ = t.args()
        assert len({x[0] for x in pico_amd.plan_shards(packed, [f or 0 for f in flat], nb, P, dir)}) == 3
        pico_amd.copy_shards(packed, flat, nb, P, dir)
        torch.cuda.synchronize()
        t.check()
    pico_amd.copy_shards(None, [], [], 2, 0)                    # n == 0: success, no launch
    pico_amd.copy_shards(None, [None, None], [0, 0], 2, 1)
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.copy_shards(t.packed.data_ptr(), [None], [4], 2, 0)
    assert ei.value.status == 1
    torch.cuda.synchronize()
    t.check()


def test_copy_shards_back_to_back(dev):
    """two calls with different tables on one stream, no synchronization in
    between, the first call's host arrays gone before the second is issued"""
    (ta, pa), (tb, pb) = mixed_tensors(3), mixed_tensors(4)
    a, b = ShardTable(ta, 3, pa, 0), ShardTable(list(reversed(tb)), 2, pb, 1)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        args = a.args()
        pico_amd.copy_shards(*args)
        del args
        pico_amd.copy_shards(*b.args())
    st.synchronize()
    a.check()
    b.check()


# ---- the two collectives over loopback ranks ---------------------------------------------------

COUNTS = [0, 1, 5, 1023, 1024, 8193, 40000]
B = sum(COUNTS)
OFF = [sum(COUNTS[:k]) for k in range(len(COUNTS))]
NP = {"float": np.float32, "int32": np.int32, "float16": np.uint16, "bfloat16": np.uint16}
GUARD = 0xA5
# (dtype, op, scale, wide); scale "1/P" is resolved per P, op "avg" by the Python layer
RS_ROWS = [("float", "sum", None, False), ("int32", "bxor", None, False), ("float", "sum", "1/P", False),
           ("bfloat16", "avg", None, True)]
RS_ALGOS = {2: ["bine_permute_remap", "bine_send_remap", "ring"], 3: ["ring"],
            4: ["bine_permute_remap", "bine_send_remap", "ring"]}
AG_ALGOS = ["ring", "bine_send_remap", "bine_permute_remap", "recursivedoubling"]


class Tensors:
    """one rank's n tensors in one arena of guard bytes: tensor k starts one
    element past a 16-B boundary, with at least 16 guard bytes on either side"""

    def __init__(self, counts, esz, data=None):
        self.esz, self.counts, self.off = esz, counts, []
        o = 0
        for c in counts:
            self.off.append(o + 16 + esz)
            o = (o + 16 + esz + c * esz + 16 + 15) & ~15
        self.host = np.full(o + 16, GUARD, dtype=np.uint8)
        if data is not None:
            for c, f, x in zip(counts, self.off, data):
                self.host[f:f + c * esz] = np.ascontiguousarray(x).view(np.uint8)
        self.t = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0

    def ptrs(self, at=None):
        """the tensors' addresses (at: an element offset per tensor)"""
        return [self.t.data_ptr() + f + (at[k] * self.esz if at else 0) for k, f in enumerate(self.off)]

    def read(self, counts=None, at=None):
        """(per tensor, `counts[k]` elements from element at[k] as bytes; whether
        every other byte of the arena is as it was)"""
        counts = self.counts if counts is None else counts
        got = self.t.cpu().numpy()
        mask = np.zeros(got.size, dtype=bool)
        parts = []
        for k, (c, f) in enumerate(zip(counts, self.off)):
            f += at[k] * self.esz if at else 0
            mask[f:f + c * self.esz] = True
            parts.append(got[f:f + c * self.esz].copy())
        return parts, bool(np.array_equal(got[~mask], self.host[~mask]))


def equal(got, exp, dtype):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if dtype in H.TYPES:
        return H.same(got.view(np.uint16), exp.view(np.uint16), dtype)
    return np.array_equal(got.view(np.uint8), exp.view(np.uint8))


def rs_inputs(dtype, op, P):
    """per rank: M, the rank-major packed buffer of P blocks of B elements"""
    if dtype in H.TYPES:
        return H.inputs(dtype, P * B, P, "sum" if op == "avg" else op)
    return O.inputs(dtype, P * B, P)


def flat_of(M, P, k):
    """tensor k of the rank whose packed buffer is M: its P shards one after another"""
    return np.concatenate([M[j * B + OFF[k]:j * B + OFF[k] + COUNTS[k]] for j in range(P)])


def rs_single(cs, algo, Ms, dtype, op, scale, wide):
    """the yardstick: the existing single call, out of place on the host-packed buffer"""
    P = len(Ms)
    ds = [TG.to_dev(x, pad=64) for x in Ms]
    dr = [torch.full((B * Ms[0].dtype.itemsize + 64,), GUARD, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
    torch.cuda.synchronize()
    f = pico_amd.loopback_reduce_scatter_wide if wide else pico_amd.loopback_reduce_scatter
    _, st = f(cs, algo, ds, dr, [B] * P, dtype, op, scale=scale)
    torch.cuda.synchronize()
    return [d[:B * x.dtype.itemsize].cpu().numpy().view(x.dtype).copy() for d, x in zip(dr, Ms)], st


def rs_multi(cs, algo, Ms, dtype, op, scale, wide, alias):
    """one loopback_reduce_scatter_multi call; alias: rbufs[k] is the head of
    sbufs[k].  Returns (per-rank outputs as one array of B elements, statuses,
    problems)"""
    P, esz = len(Ms), Ms[0].dtype.itemsize
    full = [P * c for c in COUNTS]
    inp = [Tensors(full, esz, [flat_of(M, P, k) for k in range(len(COUNTS))]) for M in Ms]
    out = inp if alias else [Tensors(COUNTS, esz) for _ in range(P)]
    torch.cuda.synchronize()
    _, st = pico_amd.loopback_reduce_scatter_multi(cs, algo, [t.ptrs() for t in inp], [t.ptrs() for t in out], dtype,
                                                   op, shard_counts=COUNTS, scale=scale, wide=wide)
    torch.cuda.synchronize()
    res, problems = [], []
    for r in range(P):
        parts, guards = out[r].read(COUNTS)
        res.append(np.concatenate(parts).view(Ms[0].dtype))
        if not guards:     # alias: the rest of every sbuf counts as surroundings too
            problems.append(f"rank {r}: bytes around an rbuf changed")
        if not alias and not np.array_equal(inp[r].t.cpu().numpy(), inp[r].host):
            problems.append(f"rank {r}: an sbuf changed")
    return res, st, problems


@pytest.mark.parametrize("P", [2, 3, 4])
def test_reduce_scatter_multi_equals_the_single_call(dev, P):
    bad, compared = [], 0
    cs = TG.comms(P)
    for algo in RS_ALGOS[P]:
        for dtype, op, scale, wide in RS_ROWS:
            scale = 1.0 / P if scale == "1/P" else scale
            Ms = [np.ascontiguousarray(x).view(NP[dtype]) for x in rs_inputs(dtype, op, P)]
            exp, est = rs_single(cs, algo, Ms, dtype, op, scale, wide)
            case = (algo, dtype, op, scale, wide)
            if any(est):
                bad.append((case, "the single call refuses", est))
                continue
            if (dtype, op, scale) == ("float", "sum", None):
                want, _ = O.reduce_scatter(algo, Ms, [B] * P, dtype)
                if not all(np.array_equal(exp[r], want[r]) for r in range(P)):
                    bad.append((case, "the single call differs from the oracle"))
            for alias in (False, True):
                got, st, problems = rs_multi(cs, algo, Ms, dtype, op, scale, wide, alias)
                if st != est:
                    bad.append((case, alias, "status", st, est))
                else:
                    compared += 1
                    if not all(equal(got[r], exp[r], dtype) for r in range(P)):
                        bad.append((case, alias, "bits"))
                bad += [(case, alias, p) for p in problems]
    assert not bad, bad[:8]
    assert compared == len(RS_ALGOS[P]) * len(RS_ROWS) * 2, compared


@pytest.mark.parametrize("P", [2, 3, 4])
def test_allgather_multi_is_concatenation(dev, P):
    """out of place, sbufs=None (every tensor's input at its own place in rbufs),
    and sbufs[k] a view into rbufs[k] (at another rank's place for odd k)"""
    bad, compared, supported = [], 0, set()
    cs = TG.comms(P)
    for dtype in ("float", "bfloat16"):
        esz = np.dtype(NP[dtype]).itemsize
        xs = O.inputs("float", B, P) if dtype == "float" else H.inputs(dtype, B, P)
        shards = [[np.ascontiguousarray(x).view(NP[dtype])[o:o + c] for o, c in zip(OFF, COUNTS)] for x in xs]
        want = [np.concatenate([shards[j][k] for j in range(P)]).view(np.uint8) for k in range(len(COUNTS))]
        full = [P * c for c in COUNTS]
        for algo in AG_ALGOS:
            # whether the single call delivers this P
            probe_s = [TG.to_dev(np.arange(4, dtype=np.float32)) for _ in range(P)]
            probe_r = [torch.zeros(16 * P + 64, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
            _, est = pico_amd.loopback_allgather(cs, algo, probe_s, probe_r, 4, "float")
            torch.cuda.synchronize()
            if not any(est):
                supported.add(algo)
            for mode in ("out", "none", "view"):
                out = [Tensors(full, esz) for _ in range(P)]
                if mode == "out":
                    inp = [Tensors(COUNTS, esz, shards[r]) for r in range(P)]
                    sbufs = [t.ptrs() for t in inp]
                else:
                    # rank r's shard of tensor k inside its own rbufs[k]: at its own
                    # place, or (view, odd k) at the next rank's place
                    at = [[((r + 1) % P if mode == "view" and k % 2 else r) * c for k, c in enumerate(COUNTS)]
                          for r in range(P)]
                    for r in range(P):
                        for k, c in enumerate(COUNTS):
                            f = out[r].off[k] + at[r][k] * esz
                            out[r].host[f:f + c * esz] = shards[r][k].view(np.uint8)
                        out[r].t.copy_(torch.from_numpy(out[r].host))
                    sbufs = None if mode == "none" else [out[r].ptrs(at[r]) for r in range(P)]
                torch.cuda.synchronize()
                _, st = pico_amd.loopback_allgather_multi(cs, algo, sbufs, [t.ptrs() for t in out], dtype,
                                                          shard_counts=COUNTS)
                torch.cuda.synchronize()
                case = (dtype, algo, mode)
                if st != est:
                    bad.append((case, "status", st, est))
                    continue
                if any(est):
                    continue
                compared += 1
                for r in range(P):
                    parts, guards = out[r].read()
                    if not all(np.array_equal(p, w) for p, w in zip(parts, want)):
                        bad.append((case, r, "bytes"))
                    if not guards:
                        bad.append((case, r, "bytes around an rbuf changed"))
                    if mode == "out" and not np.array_equal(inp[r].t.cpu().numpy(), inp[r].host):
                        bad.append((case, r, "an sbuf changed"))
    assert not bad, bad[:8]
    print(f"P={P}: {compared} calls compared")
    # 2 types x 3 modes per algorithm the single call delivers at this P: all four
    # at a power of two, ring at every P
    assert "ring" in supported and (P & (P - 1) or len(supported) == len(AG_ALGOS)), supported
    assert compared == 6 * len(supported), compared


def test_one_tensor_and_statuses(dev):
    P = 2
    cs = TG.comms(P)
    c = 40000
    # reduce-scatter: one non-empty tensor, no overlap -- the single call on the caller's own buffers
    Ms = O.inputs("float", P * c, P)
    ds = [TG.to_dev(x, pad=64) for x in Ms]
    dr = [torch.full((c * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
    _, est = pico_amd.loopback_reduce_scatter(cs, "bine_permute_remap", ds, dr, [c] * P, "float")
    torch.cuda.synchronize()
    exp = [d[:c * 4].cpu().numpy().copy() for d in dr]
    inp = [Tensors([0, P * c, 0], 4, [x[:0], x, x[:0]]) for x in Ms]
    out = [Tensors([0, c, 0], 4) for _ in range(P)]
    rc, st = pico_amd.loopback_reduce_scatter_multi(cs, "bine_permute_remap", [t.ptrs() for t in inp],
                                                    [t.ptrs() for t in out], "float", shard_counts=[0, c, 0])
    torch.cuda.synchronize()
    assert rc == 0 and st == est == [0] * P
    for r in range(P):
        parts, guards = out[r].read()
        assert guards and np.array_equal(parts[1], exp[r])
    # allgather: likewise
    xs = O.inputs("float", c, P)
    ds = [TG.to_dev(x, pad=64) for x in xs]
    dr = [torch.full((P * c * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
    _, est = pico_amd.loopback_allgather(cs, "bine_send_remap", ds, dr, c, "float")
    torch.cuda.synchronize()
    exp = [d[:P * c * 4].cpu().numpy().copy() for d in dr]
    assert np.array_equal(exp[0], np.concatenate(xs).view(np.uint8))
    inp = [Tensors([c], 4, [x]) for x in xs]
    out = [Tensors([P * c], 4) for _ in range(P)]
    rc, st = pico_amd.loopback_allgather_multi(cs, "bine_send_remap", [t.ptrs() for t in inp],
                                               [t.ptrs() for t in out], "float", shard_counts=[c])
    torch.cuda.synchronize()
    assert rc == 0 and st == est == [0] * P
    for r in range(P):
        parts, guards = out[r].read()
        assert guards and np.array_equal(parts[0], exp[r])
    before = [t.t.clone() for t in out]
    # B == 0 and n == 0: success, nothing written
    for counts in ([0], []):
        bufs = [t.ptrs()[:len(counts)] for t in out]
        rc, st = pico_amd.loopback_allgather_multi(cs, "ring", None, bufs, "float", shard_counts=counts)
        assert rc == 0 and st == [0] * P
        rc, st = pico_amd.loopback_reduce_scatter_multi(cs, "ring", bufs, bufs, "float", shard_counts=counts)
        assert rc == 0 and st == [0] * P
    # a NULL buffer with a non-zero count: BINE_ERR_ARG on every rank, nothing written
    rc, st = pico_amd.loopback_allgather_multi(cs, "ring", None, [[None], out[1].ptrs()], "float", shard_counts=[c])
    assert rc == 1 and st == [1] * P
    rc, st = pico_amd.loopback_reduce_scatter_multi(cs, "ring", [[None], out[1].ptrs()], [t.ptrs() for t in out],
                                                    "float", shard_counts=[c])
    assert rc == 1 and st == [1] * P
    # an algorithm id outside the range: what the single call returns
    rc, st = pico_amd.loopback_allgather_multi(cs, 999, None, [t.ptrs() for t in out], "float", shard_counts=[c])
    assert st == [6] * P
    rc, st = pico_amd.loopback_reduce_scatter_multi(cs, 999, [t.ptrs() for t in out], [t.ptrs() for t in out],
                                                    "float", shard_counts=[c])
    assert st == [6] * P
    torch.cuda.synchronize()
    assert all(torch.equal(t.t, b) for t, b in zip(out, before))
