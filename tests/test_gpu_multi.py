"""Multi-buffer allreduce on the GPU: the segmented copy (bine_copy_segments /
k_copy_segs) against the host, and bine_allreduce_multi over loopback ranks on
one GPU, bit for bit against the existing single call run in place on the
concatenation (loopback_allreduce / loopback_allreduce_wide: not new code) and,
for float SUM, against the oracle."""
import os

import numpy as np
import pytest

import h16_util as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402

SIZES = [0, 1, 15, 16, 17, 4095, (32 << 10) - 1, 32 << 10, (32 << 10) + 1, (1 << 20) + 3]
TILE = 32 << 10
S = _lib.COPY_SEGS_PER_LAUNCH


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- bine_copy_segments ------------------------------------------------------------------

class Table:
    """segments (dst phase, src phase, bytes, null) carved out of one source and
    one destination arena filled with two different patterns; every range has
    at least 16 guard bytes of the arena's own pattern directly before and
    after it"""

    def __init__(self, segs):
        self.segs = segs
        self.doff, self.soff = [], []
        d = s = 0
        for dp, sp, nb, _ in segs:
            self.doff.append(d + 16 + dp)
            self.soff.append(s + 16 + sp)
            d = (d + 16 + dp + nb + 16 + 15) & ~15
            s = (s + 16 + sp + nb + 16 + 15) & ~15
        self.src_host = ((np.arange(s + 16, dtype=np.uint64) * 7 + 3) % 251).astype(np.uint8)
        self.dst_host = ((np.arange(d + 16, dtype=np.uint64) * 13 + 5) % 241 + 1).astype(np.uint8) | np.uint8(0x80)
        self.src = torch.from_numpy(self.src_host.copy()).to("cuda:0")
        self.dst = torch.from_numpy(self.dst_host.copy()).to("cuda:0")
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        self.want = self.dst_host.copy()
        for (dp, sp, nb, null), do, so in zip(segs, self.doff, self.soff):
            self.want[do:do + nb] = self.src_host[so:so + nb]

    def args(self):
        dsts = [None if null else self.dst.data_ptr() + do for (_, _, _, null), do in zip(self.segs, self.doff)]
        srcs = [None if null else self.src.data_ptr() + so for (_, _, _, null), so in zip(self.segs, self.soff)]
        return dsts, srcs, [nb for _, _, nb, _ in self.segs]

    def check(self):
        got = self.dst.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:4]}"
        assert np.array_equal(self.src.cpu().numpy(), self.src_host)


def mixed_segments(seed):
    """about 40 segments: every size at a random phase pair, zero-length ones
    in between (some with NULL pointers), one of several tiles and a ragged tail"""
    rng = np.random.default_rng(seed)
    segs = []
    for rep in range(4):
        for nb in SIZES:
            if nb > (1 << 20) and rep:
                continue
            segs.append((int(rng.integers(0, 16)), int(rng.integers(0, 16)), nb, nb == 0 and rep == 1))
        segs.append((0, 0, 0, True))
    segs.insert(5, (3, 9, 5 * TILE + 777, False))      # not co-aligned, 6 workgroups
    segs.insert(11, (6, 6, 3 * TILE + 16 + 5, False))  # co-aligned off a 16-B boundary
    segs.insert(17, (0, 0, 4 * TILE, False))           # whole tiles, aligned
    return segs


def test_copy_segments_against_host(dev):
    t = Table(mixed_segments(1))
    assert 35 <= len(t.segs) <= 45
    pico_amd.copy_segments(*t.args())
    torch.cuda.synchronize()
    t.check()


@pytest.mark.parametrize("size", [17, 4095, TILE + 1])
def test_copy_segments_every_phase_pair(dev, size):
    """all 16 x 16 (destination phase, source phase) pairs: 256 segments, two launches"""
    t = Table([(dp, sp, size, False) for dp in range(16) for sp in range(16)])
    pico_amd.copy_segments(*t.args())
    torch.cuda.synchronize()
    t.check()


def test_copy_segments_more_than_one_launch(dev):
    """non-empty segments > S with empties in between: ceil(nonempty / S) launches"""
    rng = np.random.default_rng(2)
    segs = []
    for k in range(2 * S + 37):
        segs.append((int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.choice([1, 15, 16, 17, 100, 4095])),
                     False))
        if k % 5 == 0:
            segs.append((0, 0, 0, k % 10 == 0))
    t = Table(segs)
    dsts, srcs, nb = t.args()
    assert len({x[0] for x in pico_amd.plan_segments([d or 0 for d in dsts], [s or 0 for s in srcs], nb)}) == 3
    pico_amd.copy_segments(dsts, srcs, nb)
    torch.cuda.synchronize()
    t.check()
    pico_amd.copy_segments([], [], [])                       # n == 0: success, no launch
    pico_amd.copy_segments([None, None], [None, None], [0, 0])
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.copy_segments([None], [t.src.data_ptr()], [4])
    assert ei.value.status == 1
    torch.cuda.synchronize()
    t.check()


def test_copy_segments_back_to_back(dev):
    """two calls with different tables on one stream, no synchronization in
    between, the first call's host arrays gone before the second is issued:
    the descriptors travel with each launch"""
    a, b = Table(mixed_segments(3)), Table(list(reversed(mixed_segments(4))))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        args = a.args()
        pico_amd.copy_segments(*args)
        del args
        pico_amd.copy_segments(*b.args())
    st.synchronize()
    a.check()
    b.check()


# ---- bine_allreduce_multi over loopback ranks -----------------------------------------------------

COUNTS = [5, 0, 1, 64, 8191, 3, 257]
TOTAL = sum(COUNTS)
ALGOS = ["bine_bdw_remap", "bine_lat", "recursivedoubling"]
# (dtype, op, scale, wide); scale "1/P" is resolved per P, op "avg" by the Python layer
ROWS = [("float", "sum", None, False), ("int32", "bxor", None, False), ("double", "max", None, False),
        ("float", "sum", 1 / 3, False), ("bfloat16", "sum", None, False),
        ("float16", "avg", None, True), ("bfloat16", "avg", None, True)]
NP = {"float": np.float32, "int32": np.int32, "double": np.float64, "float16": np.uint16, "bfloat16": np.uint16}
GUARD = 0xA5


def set_form(cs, flat):
    for c in cs:
        c.set_flat_rs(flat)
        c.set_flat_ag(2 if flat else 0)
        c.set_chunk(4096 if flat else 0)


def inputs(dtype, op, P):
    if dtype in H.TYPES:
        return H.inputs(dtype, TOTAL, P, "sum" if op == "avg" else op)
    return O.inputs(dtype, TOTAL, P)


def single(cs, algo, sb, dtype, op, scale, wide):
    """the yardstick: the existing single call, IN_PLACE on the concatenation"""
    dc = [TG.to_dev(x, pad=64) for x in sb]
    torch.cuda.synchronize()
    if wide:
        _, st = pico_amd.loopback_allreduce_wide(cs, algo, [pico_amd.IN_PLACE] * len(sb), dc, TOTAL, dtype, op,
                                                 scale=scale)
    else:
        _, st = pico_amd.loopback_allreduce(cs, algo, [pico_amd.IN_PLACE] * len(sb), dc, TOTAL, dtype, op,
                                            scale=scale)
    torch.cuda.synchronize()
    return [d[:x.nbytes].cpu().numpy().view(x.dtype).copy() for d, x in zip(dc, sb)], st


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
            raw, e = np.ascontiguousarray(data).view(np.uint8), 0
            for c, f in zip(counts, self.off):
                self.host[f:f + c * esz] = raw[e:e + c * esz]
                e += c * esz
        self.t = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0

    def ptrs(self):
        return [self.t.data_ptr() + f for f in self.off]

    def read(self):
        """(the tensors' bytes concatenated, whether every other byte of the arena is as it was)"""
        got = self.t.cpu().numpy()
        mask = np.zeros(got.size, dtype=bool)
        parts = []
        for c, f in zip(self.counts, self.off):
            mask[f:f + c * self.esz] = True
            parts.append(got[f:f + c * self.esz])
        return np.concatenate(parts), bool(np.array_equal(got[~mask], self.host[~mask]))


def multi(cs, algo, sb, dtype, op, scale, wide, mode):
    """one loopback_allreduce_multi call; mode 'out' / 'in' / 'mixed'.  Returns
    (per-rank outputs, statuses, problems)"""
    P, esz = len(sb), sb[0].dtype.itemsize
    inp = [Tensors(COUNTS, esz, x) for x in sb]
    if mode == "in":
        out, sbufs = inp, None
    elif mode == "out":
        out = [Tensors(COUNTS, esz) for _ in range(P)]
        sbufs = [t.ptrs() for t in inp]
    else:   # even segments in place (by the same pointer, or IN_PLACE), odd ones out of place
        out = [Tensors(COUNTS, esz, x) for x in sb]
        sbufs = [[(o if k % 4 == 0 else pico_amd.IN_PLACE) if k % 2 == 0 else i
                  for k, (i, o) in enumerate(zip(ti.ptrs(), to.ptrs()))] for ti, to in zip(inp, out)]
    torch.cuda.synchronize()
    _, st = pico_amd.loopback_allreduce_multi(cs, algo, sbufs, [t.ptrs() for t in out], dtype, op, counts=COUNTS,
                                              scale=scale, wide=wide)
    torch.cuda.synchronize()
    res, problems = [], []
    for r in range(P):
        raw, guards = out[r].read()
        res.append(raw.view(sb[0].dtype))
        if not guards:
            problems.append(f"rank {r}: bytes around an rbuf changed")
        if mode != "in":
            raw, guards = inp[r].read()
            if not guards or not np.array_equal(raw, np.ascontiguousarray(sb[r]).view(np.uint8)):
                problems.append(f"rank {r}: an sbuf changed")
    return res, st, problems


def equal(got, exp, dtype):
    if dtype in H.TYPES:
        return H.same(got, exp, dtype)
    return np.array_equal(got.view(np.uint8), exp.view(np.uint8))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_allreduce_multi_equals_the_single_call(dev, P):
    bad, compared = [], 0
    cs = TG.comms(P)
    saved = os.environ.get("BINE_WIDE_TREES")
    try:
        for flat in (False, True):
            set_form(cs, flat)
            for algo in ALGOS:
                for dtype, op, scale, wide in ROWS:
                    sb = [np.ascontiguousarray(x).view(NP[dtype]) for x in inputs(dtype, op, P)]
                    for trees in ((None, "0") if wide else (None,)):
                        if trees is None:
                            os.environ.pop("BINE_WIDE_TREES", None)
                        else:
                            os.environ["BINE_WIDE_TREES"] = trees
                        exp, est = single(cs, algo, sb, dtype, op, scale, wide)
                        case = (flat, algo, dtype, op, scale, wide, trees)
                        if not any(est) and (dtype, op, scale) == ("float", "sum", None):
                            want, _ = O.allreduce(algo, sb, dtype)
                            if not all(np.array_equal(exp[r], want[r]) for r in range(P)):
                                bad.append((case, "the single call differs from the oracle"))
                        for mode in ("out", "in", "mixed"):
                            got, st, problems = multi(cs, algo, sb, dtype, op, scale, wide, mode)
                            if st != est:
                                bad.append((case, mode, "status", st, est))
                            elif not any(est):
                                compared += 1
                                if not all(equal(got[r], exp[r], dtype) for r in range(P)):
                                    bad.append((case, mode, "bits"))
                            bad += [(case, mode, p) for p in problems]
    finally:
        set_form(cs, False)
        if saved is None:
            os.environ.pop("BINE_WIDE_TREES", None)
        else:
            os.environ["BINE_WIDE_TREES"] = saved
    assert not bad, bad[:8]
    # 2 forms x 3 algorithms x (5 rows + 2 wide rows x 2 paths) x 3 modes; at P = 3 the
    # power-of-two algorithm is refused by the single call and the multi call alike
    print(f"P={P}: {compared} calls compared bit for bit")
    assert compared == (162 if P & (P - 1) == 0 else 108), compared


def test_workspace_growth(dev):
    """a small call, one that needs a larger workspace, the small one again"""
    P = 4
    cs = pico_amd.Comm.loopback(P, 0)    # a fresh group: its workspace starts empty
    try:
        for counts in ([100, 3, 29], [70001, 5, 300000], [100, 3, 29]):
            n = sum(counts)
            sb = O.inputs("float", n, P)
            want, _ = O.allreduce("bine_bdw_remap", sb, "float")
            ts = [Tensors(counts, 4, x) for x in sb]
            torch.cuda.synchronize()
            rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_bdw_remap", None, [t.ptrs() for t in ts], "float",
                                                       "sum", counts=counts)
            torch.cuda.synchronize()
            assert rc == 0 and st == [0] * P
            for r in range(P):
                raw, guards = ts[r].read()
                assert guards and np.array_equal(raw.view(np.float32), want[r]), (counts, r)
    finally:
        for c in cs:
            c.destroy()


def test_statuses(dev):
    P = 2
    cs = TG.comms(P)
    sb = O.inputs("float", 64, P)
    ts = [Tensors([64], 4, x) for x in sb]
    before = [t.t.clone() for t in ts]
    # a NULL buffer with a non-zero count: BINE_ERR_ARG on every rank, nothing written
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_lat", None, [[None], ts[1].ptrs()], "float", "sum",
                                               counts=[64])
    assert rc == 1 and st == [1] * P
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_lat", [[None], ts[1].ptrs()], [t.ptrs() for t in ts],
                                               "float", "sum", counts=[64])
    assert rc == 1 and st == [1] * P
    # n == 0, and every count zero: success, nothing written
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_lat", None, [[], []], "float", "sum", counts=[])
    assert rc == 0 and st == [0] * P
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_lat", None, [t.ptrs() for t in ts], "float", "sum",
                                               counts=[0])
    assert rc == 0 and st == [0] * P
    # an algorithm id outside the allreduce range: what bine_allreduce returns
    rc, st = pico_amd.loopback_allreduce_multi(cs, 999, None, [t.ptrs() for t in ts], "float", "sum", counts=[64])
    _, st1 = pico_amd.loopback_allreduce(cs, 999, [pico_amd.IN_PLACE] * P, [t.ptrs()[0] for t in ts], 64, "float")
    assert st == st1 == [6] * P
    torch.cuda.synchronize()
    assert all(torch.equal(t.t, b) for t, b in zip(ts, before))
    # n == 1 equals the single call, out of place and in place
    want, est = single(cs, "bine_bdw_remap", [np.asarray(x) for x in sb], "float", "sum", None, False)
    outs = [Tensors([64], 4) for _ in range(P)]
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_bdw_remap", [t.ptrs() for t in ts],
                                               [t.ptrs() for t in outs], "float", "sum", counts=[64])
    torch.cuda.synchronize()
    assert rc == 0 and st == est == [0] * P
    for r in range(P):
        raw, guards = outs[r].read()
        assert guards and np.array_equal(raw.view(np.float32), want[r])
    rc, st = pico_amd.loopback_allreduce_multi(cs, "bine_bdw_remap", None, [t.ptrs() for t in ts], "float", "sum",
                                               counts=[64])
    torch.cuda.synchronize()
    assert rc == 0
    for r in range(P):
        raw, guards = ts[r].read()
        assert guards and np.array_equal(raw.view(np.float32), want[r])
