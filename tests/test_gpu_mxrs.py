"""MX-quantized gradient reduce-scatter on the GPU: bine_mx_sum_segments against
tests/mxrs_sim.py bit for bit on both bodies, every stream count that takes
another number of loads, every tile edge, lists across a launch cut, NaN
blocks, subnormal products and three scales; bine_mx_reduce_scatter_multi over
loopback ranks against the sim's pack + exchange + sum, against its three steps
issued one by one, in place, with an infinity planted, and against an error
bound derived from the contract.  Guard bytes surround every output and
workspace, and every source is compared untouched.  (Real processes and graph
mode: tools/mxrs_check.py, tests/test_gpu_mxrs_rccl.py.)"""
import numpy as np
import pytest

import fp8_sim as F
import h16_util as H
import mx_sim as M
import mxrs_sim as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402
from test_gpu_quant import Bucket, from_values  # noqa: E402  (the guarded arena)

S = _lib.MX_SEGS_PER_LAUNCH
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
CASES = [(d, f) for d in TYPES for f in M.FORMATS]
SCALES = (1.0, 0.25, 1.0 / 3.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tile_of(dtype):
    return 32768 // ESZ[dtype]


def random_streams(counts, fmt, ns, rng, lo=97, hi=157, finite=False):
    """ns wire blocks: random data bytes, scale bytes over 60 binades (additions
    round), pad bytes of their own; finite: no NaN and no infinity code"""
    _, _, D, B = R.layout(counts, fmt)
    nsc = sum(c // 32 for c in counts)
    out = []
    for _ in range(ns):
        b = rng.integers(0, 256, B, dtype=np.uint8)
        if finite and fmt != "e2m1":
            top = 0x7E if fmt == "e4m3" else 0x7B
            b[:D] = np.where((b[:D] & 0x7F) > top, b[:D] & 0x80 | 0x31, b[:D])
        b[D:D + nsc] = rng.integers(lo, hi, nsc, dtype=np.uint8)
        out.append(b)
    return out


def run_sum(ddtype, fmt, blocks, counts, phases, scale, nulls=None):
    """sum `blocks` into tensors of `counts` elements at `phases` (in elements off a 16-B boundary); returns the
    tensors' patterns and the plan; guards and the packed bytes checked"""
    esz, ns = ESZ[ddtype], len(blocks)
    nulls = nulls or [False] * len(counts)
    B = R.layout(counts, fmt)[3]
    packed = Bucket(1, [(max(ns * B, 16), 0, False)], [np.concatenate(blocks) if B else np.zeros(16, dtype=np.uint8)])
    dst = Bucket(esz, [(c, ph * esz, nl) for c, ph, nl in zip(counts, phases, nulls)])
    plan = pico_amd.plan_mx_sum([p or 0 for p in dst.ptrs()], counts, ddtype, fmt)
    pico_amd.mx_sum_segments(packed.ptrs()[0], ns, B, dst.ptrs(), fmt, scale=scale, ddtype=ddtype, counts=counts)
    torch.cuda.synchronize()
    got, guards = dst.read(R.VIEW[ddtype])
    assert guards, "bytes outside the destinations were written"
    assert packed.unchanged(), "the packed blocks were written"
    return got, plan


def assert_is_sim(got, blocks, counts, fmt, ddtype, scale, what):
    want = R.sum_blocks(blocks, counts, fmt, ddtype, scale)
    for k in range(len(counts)):
        bad = R.same(got[k], want[k], ddtype)
        assert bad.size == 0, (what, ddtype, fmt, len(blocks), k, bad, got[k][bad], want[k][0][bad])


# ---- bine_mx_sum_segments ----------------------------------------------------------------------

@pytest.mark.parametrize("ddtype,fmt", CASES)
def test_sum_is_the_sim_on_both_bodies(dev, ddtype, fmt):
    """every tile edge, 16-B aligned (vector body) and one element off (element body), in one call per stream count"""
    rng = np.random.default_rng(6111)
    tile = tile_of(ddtype)
    edge = [32, 64, tile - 32, tile, tile + 32, 2 * tile + 32]
    counts, phases = edge + edge, [0] * len(edge) + [1] * len(edge)
    for i, ns in enumerate((1, 2, 3, 4, 8, 16)):
        blocks = random_streams(counts, fmt, ns, rng)
        scale = SCALES[i % 3]
        got, plan = run_sum(ddtype, fmt, blocks, counts, phases, scale)
        assert [r[4] for r in plan] == phases and [r[3] for r in plan] == [1, 1, 1, 1, 2, 3] * 2
        assert_is_sim(got, blocks, counts, fmt, ddtype, scale, "edges")


@pytest.mark.parametrize("ddtype,fmt", CASES)
def test_sum_nan_block_and_subnormal_products(dev, ddtype, fmt):
    rng = np.random.default_rng(6112)
    tile = tile_of(ddtype)
    counts, phases = [tile + 64, 96], [0, 1]
    # S = 0xFF in one stream, one block per tensor: exactly those 32 quiet NaNs, nothing else
    blocks = random_streams(counts, fmt, 3, rng, 120, 134, finite=True)
    _, soff, _, _ = R.layout(counts, fmt)
    blocks[1][soff[0] + tile // 32] = 0xFF            # tensor 0: the first block of its second tile
    blocks[2][soff[1] + 1] = 0xFF                     # tensor 1: its middle block
    got, _ = run_sum(ddtype, fmt, blocks, counts, phases, 1.0)
    assert_is_sim(got, blocks, counts, fmt, ddtype, 1.0, "nan block")
    for k, b in ((0, tile // 32), (1, 1)):
        nan = R.is_nan(got[k], ddtype)
        assert nan[32 * b:32 * b + 32].all() and nan.sum() == 32
        assert (got[k][32 * b:32 * b + 32] == R.QNAN[ddtype]).all()
    # S = 0 in every stream: products down to 2^-143, float32 subnormals kept
    blocks = random_streams(counts, fmt, 4, rng, 0, 1, finite=True)
    got, _ = run_sum(ddtype, fmt, blocks, counts, phases, 1.0)
    assert_is_sim(got, blocks, counts, fmt, ddtype, 1.0, "S = 0")
    if ddtype == "float":
        mags = np.concatenate(got).view(np.uint32) & 0x7FFFFFFF
        assert ((mags > 0) & (mags < 0x00800000)).sum() > 100        # subnormal sums among them, kept


@pytest.mark.parametrize("n", [0, 1, S + 1])
def test_lists_with_empties(dev, n):
    rng = np.random.default_rng(n)
    for i, (ddtype, fmt) in enumerate((("float", "e4m3"), ("bfloat16", "e2m1"), ("float16", "e5m2"))):
        counts = [0 if k % 5 == 2 else 32 * int(rng.integers(1, 7)) for k in range(n)]
        nulls = [c == 0 and k % 2 == 0 for k, c in enumerate(counts)]
        phases = [int(k % 3 == 1) for k in range(n)]
        blocks = random_streams(counts, fmt, 3, rng)
        got, plan = run_sum(ddtype, fmt, blocks, counts, phases, SCALES[i], nulls)
        assert len(plan) == sum(c > 0 for c in counts) and len({r[0] for r in plan}) == -(-len(plan) // S)
        assert n < 2 or {r[4] for r in plan} == {0, 1}
        assert_is_sim(got, blocks, counts, fmt, ddtype, SCALES[i], "list")


# ---- bine_mx_reduce_scatter_multi --------------------------------------------------------------

SHARDS = [32, 8192 + 32, 0, 64]
COMBOS = (("float", "e4m3"), ("bfloat16", "e5m2"), ("float", "e2m1"))


def gradients(dtype, P, rng):
    """per tensor P shards: each block in a binade range of its own within 2^+-20"""
    out = []
    for c in SHARDS:
        n = P * c
        top = np.repeat(rng.integers(-20, 20, n // 32), 32)
        x = rng.standard_normal(n) * np.exp2(top - rng.integers(0, 12, n) * (rng.integers(0, 3, n) == 0))
        x[rng.integers(0, 11, n) == 0] = 0.0
        out.append(from_values(dtype, x.astype(np.float32)))
    return out


class Ranks:
    """per rank its gradients, shards and workspaces in guarded arenas; tensor 0
    stands one element off a 16-B boundary on both sides (the element bodies)"""

    def __init__(self, P, dtype, fmt, data):
        self.P, self.dtype, self.fmt, self.data = P, dtype, fmt, data
        esz = ESZ[dtype]
        self.B = R.layout(SHARDS, fmt)[3]
        self.src = [Bucket(esz, [(P * c, (k == 0) * esz, c == 0) for k, c in enumerate(SHARDS)], data[r])
                    for r in range(P)]
        self.dst = [Bucket(esz, [(c, (k == 0) * esz, c == 0) for k, c in enumerate(SHARDS)]) for _ in range(P)]
        self.sws = [Bucket(1, [(P * self.B, 0, False)]) for _ in range(P)]
        self.rws = [Bucket(1, [(P * self.B, 0, False)]) for _ in range(P)]

    def run(self, cs, rbufs=None, **kw):
        rc, st = pico_amd.loopback_mx_reduce_scatter_multi(
            cs, [b.ptrs() for b in self.src], rbufs or [b.ptrs() for b in self.dst], self.fmt, sdtype=self.dtype,
            rdtype=self.dtype, shard_counts=SHARDS, send_ws=[b.ptrs()[0] for b in self.sws],
            recv_ws=[b.ptrs()[0] for b in self.rws], **kw)
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * self.P, (rc, st)

    def results(self):
        out = []
        for r in range(self.P):
            got, guards = self.dst[r].read(R.VIEW[self.dtype])
            assert guards and self.src[r].unchanged(), r
            assert self.sws[r].read()[1] and self.rws[r].read()[1], "bytes around a workspace were written"
            out.append(got)
        return out


def assert_ranks_are(got, want, dtype, what):
    for r in range(len(got)):
        for k in range(len(SHARDS)):
            bad = R.same(got[r][k], want[r][k], dtype)
            assert bad.size == 0, (what, dtype, r, k, bad, got[r][k][bad], want[r][k][0][bad])


@pytest.mark.parametrize("P", [2, 4])
def test_reduce_scatter_is_the_sim_its_three_parts_and_in_place(dev, P):
    cs = TG.comms(P)
    for i, (dtype, fmt) in enumerate(COMBOS):
        rng = np.random.default_rng(6113 + i)
        data = [gradients(dtype, P, rng) for _ in range(P)]
        scale = (None, 0.25, None)[i]
        op = ("sum", "sum", "avg")[i]
        eff = 1.0 / P if op == "avg" else (scale or 1.0)
        want, recv = R.reduce_scatter(data, SHARDS, dtype, dtype, fmt, eff)
        fused = Ranks(P, dtype, fmt, data)
        fused.run(cs, op=op, scale=scale)
        got = fused.results()
        assert_ranks_are(got, want, dtype, "fused")
        for r in range(P):                                     # the received blocks, pad bytes aside
            rws = fused.rws[r].read()[0][0].reshape(P, fused.B)
            used = R.layout(SHARDS, fmt)[2] + sum(c // 32 for c in SHARDS)
            assert all(np.array_equal(rws[j][:used], recv[r][j][:used]) for j in range(P)), (dtype, fmt, r)
        # the three steps one by one
        parts = Ranks(P, dtype, fmt, data)
        doff, soff, _, B = R.layout(SHARDS, fmt)
        esz = ESZ[dtype]
        for r in range(P):
            pairs = [(k, j) for j in range(P) for k, c in enumerate(SHARDS) if c]
            base, sp = parts.sws[r].ptrs()[0], parts.src[r].ptrs()
            pico_amd.mx_quant_segments([sp[k] + j * SHARDS[k] * esz for k, j in pairs],
                                       [base + j * B + doff[k] for k, j in pairs],
                                       [base + j * B + soff[k] for k, j in pairs], fmt, sdtype=dtype,
                                       counts=[SHARDS[k] for k, _ in pairs])
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_alltoall(cs, "bine", [b.ptrs()[0] for b in parts.sws],
                                            [b.ptrs()[0] for b in parts.rws], B, "uint8")
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * P
        for r in range(P):
            pico_amd.mx_sum_segments(parts.rws[r].ptrs()[0], P, B, parts.dst[r].ptrs(), fmt, scale=eff, ddtype=dtype,
                                     counts=SHARDS)
        torch.cuda.synchronize()
        step = parts.results()
        for r in range(P):
            assert all(np.array_equal(a, b) for a, b in zip(got[r], step[r])), (dtype, fmt, r)
        # again with rbufs[k] = this rank's own shard of sbufs[k]
        alias = Ranks(P, dtype, fmt, data)
        own = [[None if c == 0 else p + r * c * esz for p, c in zip(alias.src[r].ptrs(), SHARDS)] for r in range(P)]
        alias.run(cs, rbufs=own, op=op, scale=scale)
        for r in range(P):
            parts_r, guards = alias.src[r].read(R.VIEW[dtype])
            assert guards
            for k, c in enumerate(SHARDS):
                full = np.ascontiguousarray(data[r][k]).view(R.VIEW[dtype]).copy()
                assert np.array_equal(parts_r[k][r * c:(r + 1) * c], got[r][k]), (dtype, fmt, r, k)
                full[r * c:(r + 1) * c] = got[r][k]
                assert np.array_equal(parts_r[k], full), "a shard of another rank was written"


@pytest.mark.parametrize("P", [2, 4])
def test_reduce_scatter_within_the_contracts_error_bound(dev, P):
    """|result - float64 sum of the inputs| <= sum_j E_fmt * 2^(S_j - 127) + (P - 1) * 2^-24 * sum_j |d_j|, plus
    one final rounding for a 16-bit output (bfloat16: 2^-9 of the float32 sum's magnitude, itself within the
    bound's first two terms of sum_j |d_j|): S_j and d_j read from the sim, no tolerance picked"""
    cs = TG.comms(P)
    for i, (dtype, fmt) in enumerate(COMBOS):
        rng = np.random.default_rng(6120 + i)
        data = [gradients(dtype, P, rng) for _ in range(P)]
        _, recv = R.reduce_scatter(data, SHARDS, dtype, dtype, fmt)
        ranks = Ranks(P, dtype, fmt, data)
        ranks.run(cs)
        got = ranks.results()
        for r in range(P):
            per = [R.values(recv[r][j], SHARDS, fmt) for j in range(P)]
            for k, c in enumerate(SHARDS):
                if c == 0:
                    continue
                wide = [F.widen(data[j][k][r * c:(r + 1) * c], dtype).astype(np.float64) for j in range(P)]
                exact = sum(wide)
                quant = sum(R.E_FMT[fmt] * np.exp2(per[j][k][1].astype(np.float64) - 127) for j in range(P))
                mag = sum(np.abs(per[j][k][0].astype(np.float64)) for j in range(P))
                bound = quant + (P - 1) * 2.0 ** -24 * mag
                if dtype != "float":
                    bound = bound + 2.0 ** -9 * (mag + bound)
                val = (got[r][k].view(np.float32) if dtype == "float" else
                       H.to_f32(got[r][k], dtype)).astype(np.float64)
                err = np.abs(val - exact)
                assert np.isfinite(val).all() and (err <= bound).all(), (dtype, fmt, r, k, float((err / bound).max()))
                assert err.max() > 0                             # a lossy path: the bound is not vacuous


def test_an_infinity_is_a_nan_block_on_its_owner_only(dev):
    P, dtype, fmt = 2, "float", "e4m3"
    cs = TG.comms(P)
    rng = np.random.default_rng(6130)
    data = [gradients(dtype, P, rng) for _ in range(P)]
    c = SHARDS[1]
    data[1][1][0 * c + 40] = np.inf                    # rank 1's contribution to rank 0's shard of tensor 1, block 1
    ranks = Ranks(P, dtype, fmt, data)
    ranks.run(cs)
    got = ranks.results()
    want, _ = R.reduce_scatter(data, SHARDS, dtype, dtype, fmt)
    assert_ranks_are(got, want, dtype, "inf")
    for r in range(P):
        for k in range(len(SHARDS)):
            nan = R.is_nan(got[r][k], dtype)
            if (r, k) == (0, 1):
                assert nan[32:64].all() and nan.sum() == 32 and (got[r][k][32:64] == R.QNAN[dtype]).all()
            else:
                assert not nan.any(), (r, k)


def test_nothing_to_do(dev):
    cs = TG.comms(2)
    rc, st = pico_amd.loopback_mx_reduce_scatter_multi(cs, [[None], [None]], [[None], [None]], "e4m3", sdtype="float",
                                                       rdtype="float", shard_counts=[0])
    assert rc == 0 and st == [0, 0]
    rc, st = pico_amd.loopback_mx_reduce_scatter_multi(cs, [[]] * 2, [[]] * 2, "e2m1", sdtype="float", rdtype="float",
                                                       shard_counts=[])
    assert rc == 0 and st == [0, 0]
