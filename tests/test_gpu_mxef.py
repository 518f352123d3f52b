"""MX quantization with an error-feedback residual on the GPU:
bine_mx_quant_ef_segments against tests/mxef_sim.py bit for bit -- data bytes,
scale bytes and residuals -- on both bodies (the element body forced by the
source's phase alone, by the residual's alone and by dst8's alone), every tile
edge, lists across a launch cut, residuals 2^+-20 times x, cancelling
residuals, binary32 subnormals at S = 0, the S = 0xFF cases and -0; eight
carried steps against the CPU test's bound; bine_mx_reduce_scatter_multi_ef
over loopback ranks against the sim, against its three steps issued one by
one, in place, over two calls that carry the residual, with an infinity
planted, and with zero residuals against bine_mx_reduce_scatter_multi.  Guard
bytes surround dst8, scl8, res and the workspaces, and every source is compared
untouched.  (Real processes and graph mode: tools/mxef_check.py,
tests/test_gpu_mxef_rccl.py.)"""
import numpy as np
import pytest

import fp8_sim as F
import mx_sim as M
import mxef_sim as E
import mxrs_sim as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402
from test_gpu_mxrs import COMBOS, SHARDS, Ranks, assert_ranks_are, gradients  # noqa: E402
from test_gpu_quant import Bucket, from_values  # noqa: E402  (the guarded arena)

S = _lib.MX_EF_SEGS_PER_LAUNCH
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
CASES = [(d, f) for d in TYPES for f in M.FORMATS]
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tile_of(dtype):
    return 32768 // ESZ[dtype]


def inputs(dtype, n, rng, special=True):
    """(x, r) of n elements: per block of 32 one kind of residual -- a small
    one, 2^20 and 2^-20 times x, one that cancels x exactly (S = 0), a binary32
    subnormal over a zero x (S = 0) -- then, with 5 blocks or more, the S = 0xFF
    cases and -0 in blocks of their own"""
    span = 12 if dtype == "float16" else 20                           # every x finite in its type
    xf = (rng.standard_normal(n) * np.exp2(np.repeat(rng.integers(-span, span, -(-n // 32)), 32)[:n])).astype(np.float32)
    xf[rng.integers(0, 9, n) == 0] = 0.0
    kind = np.repeat(rng.integers(0, 6, -(-n // 32)), 32)[:n]
    xf[kind == 4] = 0.0
    x = from_values(dtype, xf)
    w = F.widen(x, dtype)
    r = (w * (rng.standard_normal(n) * 0.05).astype(np.float32)).astype(np.float32)
    r = np.where(kind == 1, w * np.float32(2.0 ** 20), r)
    r = np.where(kind == 2, w * np.float32(2.0 ** -20), r)
    r = np.where(kind == 3, -w, r)
    sub = (rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    r = np.where(kind == 4, sub, r).astype(np.float32)
    if special and n >= 5 * 32:
        big = from_values(dtype, [FLT_MAX if dtype != "float16" else 65504.0])[0]
        x[7] = from_values(dtype, [-np.inf])[0]                       # block 0: an infinity in x
        r[32 + 31] = np.nan                                           # block 1: a NaN in r
        x[64], r[64] = big, FLT_MAX                                   # block 2: x + r overflows (float16's maximum cannot)
        x[96:128] = from_values(dtype, [-0.0])[0]                     # block 3: -0 with +0, -0 and live residuals
        r[96:112], r[112:120] = 0.0, -0.0
    return x, r


def run_ef(dtype, fmt, xs, rs, ph_src=None, ph_res=None, ph_d8=None, nulls=None):
    """one call over the list; phases in BYTES off a 16-B boundary per tensor.
    Returns (data, scales, residuals, plan); guards and sources checked."""
    esz, n = ESZ[dtype], len(xs)
    z = [0] * n
    ph_src, ph_res, ph_d8, nulls = ph_src or z, ph_res or z, ph_d8 or z, nulls or [False] * n
    counts = [x.size for x in xs]
    src = Bucket(esz, [(c, p, nl) for c, p, nl in zip(counts, ph_src, nulls)], xs)
    res = Bucket(4, [(c, p, nl) for c, p, nl in zip(counts, ph_res, nulls)], rs)
    d8 = Bucket(1, [(M.dbytes(c, fmt), p, nl) for c, p, nl in zip(counts, ph_d8, nulls)])
    sc = Bucket(1, [(M.nblk(c), 1, nl) for c, nl in zip(counts, nulls)])
    addr = lambda b: [p or 0 for p in b.ptrs()]  # noqa: E731
    plan = pico_amd.plan_mx_ef(addr(src), addr(res), addr(d8), addr(sc), counts, dtype, fmt)
    pico_amd.mx_quant_ef_segments(src.ptrs(), res.ptrs(), d8.ptrs(), sc.ptrs(), fmt, sdtype=dtype, counts=counts)
    torch.cuda.synchronize()
    assert src.unchanged(), "a source was written"
    out = []
    for b, view in ((d8, np.uint8), (sc, np.uint8), (res, np.uint32)):
        got, guards = b.read(view)
        assert guards, "bytes outside an output were written"
        out.append(got)
    return out[0], out[1], out[2], plan


def assert_is_sim(got, xs, rs, dtype, fmt, what):
    data, scl, res, _ = got
    for k, (x, r) in enumerate(zip(xs, rs)):
        wd, ws, wr = E.quant_ef(x, r, dtype, fmt)
        for name, g, w in (("scale", scl[k], ws), ("data", data[k], wd), ("residual", res[k], wr.view(np.uint32))):
            bad = np.nonzero(g != w)[0][:4]
            assert bad.size == 0, (what, name, dtype, fmt, k, x.size, bad, g[bad], w[bad])


@pytest.mark.parametrize("dtype,fmt", CASES)
def test_quant_ef_is_the_sim_on_both_bodies(dev, dtype, fmt):
    rng = np.random.default_rng(6200 + 16 * TYPES.index(dtype) + M.FORMATS.index(fmt))
    t, esz = tile_of(dtype), ESZ[dtype]
    counts = [1, 31, 32, 33, t - 32, t, t + 37, 2 * t + 32]
    pairs = [inputs(dtype, c, rng) for c in counts]
    xs, rs = [p[0] for p in pairs], [p[1] for p in pairs]
    n = len(counts)
    per = (16 // esz if fmt != "e2m1" else 8 // esz)
    got = run_ef(dtype, fmt, xs, rs)
    assert {r[4] for r in got[3]} == {0} and [r[3] for r in got[3]] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert_is_sim(got, xs, rs, dtype, fmt, "vector")
    # the S = 0xFF cases, in their blocks only (float16's largest value plus FLT_MAX does not overflow)
    S5 = got[1][5]
    assert list(S5[:4] == 0xFF) == [True, True, dtype != "float16", False]
    assert not got[2][5][:64].any() and not got[0][5][:M.dbytes(64, fmt)].any()
    assert (S5[4:] != 0xFF).all()
    # the element body, forced three ways
    for what, kw in (("src", dict(ph_src=[esz] * n)), ("res", dict(ph_res=[4 * (1 + k % 3) for k in range(n)])),
                     ("d8", dict(ph_d8=[per // 2 if k % 2 and per > 1 else 1 for k in range(n)]))):
        forced = run_ef(dtype, fmt, xs, rs, **kw)
        assert {r[4] for r in forced[3]} == {1}, what
        for a, b in zip(got[:3], forced[:3]):
            assert all(np.array_equal(p, q) for p, q in zip(a, b)), ("the element body differs", what, dtype, fmt)


def test_lists_across_the_launch_cut(dev):
    for i, (dtype, fmt) in enumerate((("float", "e2m1"), ("bfloat16", "e4m3"), ("float16", "e5m2"))):
        rng = np.random.default_rng(6230 + i)
        assert run_ef(dtype, fmt, [], [])[3] == []
        for n in (1, S + 1 + 10):                                  # ten of them empty: one past a full launch
            counts = [0 if n > 1 and k % 10 == 3 else int(rng.integers(1, 200)) for k in range(n)]
            assert n == 1 or sum(c > 0 for c in counts) == S + 1
            nulls = [c == 0 and k % 20 == 3 for k, c in enumerate(counts)]
            pairs = [inputs(dtype, c, rng, special=k % 7 == 0) for k, c in enumerate(counts)]
            xs, rs = [p[0] for p in pairs], [p[1] for p in pairs]
            got = run_ef(dtype, fmt, xs, rs, ph_src=[ESZ[dtype] * (k % 4 == 1) for k in range(n)],
                         ph_res=[4 * (k % 4 == 2) for k in range(n)], ph_d8=[k % 4 == 3 for k in range(n)], nulls=nulls)
            plan = got[3]
            assert len(plan) == sum(c > 0 for c in counts) and [r[0] for r in plan] == ([0] * S + [1])[:len(plan)]
            assert n == 1 or {r[4] for r in plan} == {0, 1}
            assert_is_sim(got, xs, rs, dtype, fmt, "list")


@pytest.mark.parametrize("dtype,fmt", COMBOS)
def test_eight_carried_steps(dev, dtype, fmt):
    """sum_t d_t + r_T against sum_t widen(x) within sum_t ulp(v_t) / 2: only the additions round"""
    rng = np.random.default_rng(6240)
    n, T, esz = tile_of(dtype) + 37, 8, ESZ[dtype]
    x = from_values(dtype, (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32))
    src = Bucket(esz, [(n, 0, False)], [x])
    res = Bucket(4, [(n, 0, False)], [np.zeros(n, dtype=np.float32)])
    d8 = Bucket(1, [(M.dbytes(n, fmt), 0, False)])
    sc = Bucket(1, [(M.nblk(n), 0, False)])
    tot, slack = np.zeros(n), np.zeros(n)
    r = np.zeros(n, dtype=np.float32)
    for _ in range(T):
        v = E.add(x, r, dtype)
        want = E.quant_ef(x, r, dtype, fmt)
        pico_amd.mx_quant_ef_segments(src.ptrs(), res.ptrs(), d8.ptrs(), sc.ptrs(), fmt, sdtype=dtype, counts=[n])
        torch.cuda.synchronize()
        data, Sb, r = d8.read()[0][0], sc.read()[0][0], res.read(np.float32)[0][0]
        assert np.array_equal(data, want[0]) and np.array_equal(Sb, want[1])
        assert np.array_equal(r.view(np.uint32), want[2].view(np.uint32))
        tot += M.dequant(data, Sb, n, fmt, "float").astype(np.float64)
        slack += np.spacing(np.abs(v)).astype(np.float64) / 2
    assert src.unchanged() and d8.read()[1] and sc.read()[1] and res.read()[1]
    err = np.abs(tot + r.astype(np.float64) - T * F.widen(x, dtype).astype(np.float64))
    assert (err <= slack).all(), float((err / slack).max())
    assert np.abs(r).max() > 0


# ---- bine_mx_reduce_scatter_multi_ef -----------------------------------------------------------

class EfRanks(Ranks):
    """test_gpu_mxrs.Ranks with a guarded residual per gradient; tensor 0's stands 4 bytes off a 16-B boundary"""

    def __init__(self, P, dtype, fmt, data, res):
        super().__init__(P, dtype, fmt, data)
        self.res = [Bucket(4, [(P * c, (k == 0) * 4, c == 0) for k, c in enumerate(SHARDS)], res[r]) for r in range(P)]

    def run(self, cs, rbufs=None, **kw):
        rc, st = pico_amd.loopback_mx_reduce_scatter_multi_ef(
            cs, [b.ptrs() for b in self.src], [b.ptrs() for b in self.res], rbufs or [b.ptrs() for b in self.dst],
            self.fmt, sdtype=self.dtype, rdtype=self.dtype, shard_counts=SHARDS,
            send_ws=[b.ptrs()[0] for b in self.sws], recv_ws=[b.ptrs()[0] for b in self.rws], **kw)
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * self.P, (rc, st)

    def residuals(self):
        out = []
        for r in range(self.P):
            got, guards = self.res[r].read(np.uint32)
            assert guards, "bytes around a residual were written"
            out.append(got)
        return out


def residuals_for(data, dtype, rng):
    return [[(F.widen(x, dtype) * (rng.standard_normal(x.size) * 0.1).astype(np.float32)).astype(np.float32)
             for x in rank] for rank in data]


def assert_residuals_are(got, want, what):
    for r in range(len(got)):
        for k in range(len(SHARDS)):
            assert np.array_equal(got[r][k], want[r][k].view(np.uint32)), (what, r, k)


@pytest.mark.parametrize("P", [2, 4])
def test_reduce_scatter_ef_is_the_sim_its_three_parts_in_place_and_carries(dev, P):
    cs = TG.comms(P)
    for i, (dtype, fmt) in enumerate(COMBOS):
        rng = np.random.default_rng(6250 + i)
        data = [gradients(dtype, P, rng) for _ in range(P)]
        res = residuals_for(data, dtype, rng)
        scale, op = (None, 0.25, None)[i], ("sum", "sum", "avg")[i]
        eff = 1.0 / P if op == "avg" else (scale or 1.0)
        want, new, recv = E.reduce_scatter_ef(data, res, SHARDS, dtype, dtype, fmt, eff)
        fused = EfRanks(P, dtype, fmt, data, res)
        fused.run(cs, op=op, scale=scale)
        got = fused.results()
        assert_ranks_are(got, want, dtype, "fused")
        assert_residuals_are(fused.residuals(), new, "fused")
        used = R.layout(SHARDS, fmt)[2] + sum(c // 32 for c in SHARDS)
        for r in range(P):                                     # the received blocks, pad bytes aside
            rws = fused.rws[r].read()[0][0].reshape(P, fused.B)
            assert all(np.array_equal(rws[j][:used], recv[r][j][:used]) for j in range(P)), (dtype, fmt, r)
        # a second call carries the first one's residuals (the same gradients again)
        want2, new2, _ = E.reduce_scatter_ef(data, new, SHARDS, dtype, dtype, fmt, eff)
        fused.run(cs, op=op, scale=scale)
        assert_ranks_are(fused.results(), want2, dtype, "carried")
        assert_residuals_are(fused.residuals(), new2, "carried")
        # the three steps one by one
        parts = EfRanks(P, dtype, fmt, data, res)
        doff, soff, _, B = R.layout(SHARDS, fmt)
        esz = ESZ[dtype]
        for r in range(P):
            pairs = [(k, j) for j in range(P) for k, c in enumerate(SHARDS) if c]
            base, sp, rp = parts.sws[r].ptrs()[0], parts.src[r].ptrs(), parts.res[r].ptrs()
            pico_amd.mx_quant_ef_segments([sp[k] + j * SHARDS[k] * esz for k, j in pairs],
                                          [rp[k] + j * SHARDS[k] * 4 for k, j in pairs],
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
        assert_residuals_are(parts.residuals(), new, "parts")
        # again with rbufs[k] = this rank's own shard of sbufs[k]
        alias = EfRanks(P, dtype, fmt, data, res)
        own = [[None if c == 0 else p + r * c * esz for p, c in zip(alias.src[r].ptrs(), SHARDS)] for r in range(P)]
        alias.run(cs, rbufs=own, op=op, scale=scale)
        assert_residuals_are(alias.residuals(), new, "in place")
        for r in range(P):
            parts_r, guards = alias.src[r].read(R.VIEW[dtype])
            assert guards
            for k, c in enumerate(SHARDS):
                full = np.ascontiguousarray(data[r][k]).view(R.VIEW[dtype]).copy()
                assert np.array_equal(parts_r[k][r * c:(r + 1) * c], got[r][k]), (dtype, fmt, r, k)
                full[r * c:(r + 1) * c] = got[r][k]
                assert np.array_equal(parts_r[k], full), "a shard of another rank was written"


@pytest.mark.parametrize("P", [2, 4])
def test_zero_residuals_give_the_plain_reduce_scatter(dev, P):
    cs = TG.comms(P)
    for i, (dtype, fmt) in enumerate(COMBOS):
        rng = np.random.default_rng(6260 + i)
        data = [gradients(dtype, P, rng) for _ in range(P)]              # no -0 among them
        assert not any((np.ascontiguousarray(x).view(R.VIEW[dtype]) == (0x80000000 if dtype == "float" else 0x8000)).any()
                       for rank in data for x in rank)
        zero = [[np.zeros(x.size, dtype=np.float32) for x in rank] for rank in data]
        ef = EfRanks(P, dtype, fmt, data, zero)
        ef.run(cs)
        plain = Ranks(P, dtype, fmt, data)
        plain.run(cs)
        a, b = ef.results(), plain.results()
        for r in range(P):
            assert all(np.array_equal(x, y) for x, y in zip(a[r], b[r])), (dtype, fmt, r)
            used = R.layout(SHARDS, fmt)[2] + sum(c // 32 for c in SHARDS)
            x, y = ef.rws[r].read()[0][0].reshape(P, ef.B), plain.rws[r].read()[0][0].reshape(P, ef.B)
            assert np.array_equal(x[:, :used], y[:, :used])


def test_an_infinity_is_a_nan_block_on_its_owner_and_a_zero_residual_on_its_sender(dev):
    P, dtype, fmt = 2, "float", "e4m3"
    cs = TG.comms(P)
    rng = np.random.default_rng(6270)
    data = [gradients(dtype, P, rng) for _ in range(P)]
    res = residuals_for(data, dtype, rng)
    c = SHARDS[1]
    data[1][1][0 * c + 40] = np.inf                    # rank 1's contribution to rank 0's shard of tensor 1, block 1
    ranks = EfRanks(P, dtype, fmt, data, res)
    ranks.run(cs)
    got = ranks.results()
    want, new, _ = E.reduce_scatter_ef(data, res, SHARDS, dtype, dtype, fmt)
    assert_ranks_are(got, want, dtype, "inf")
    rr = ranks.residuals()
    assert_residuals_are(rr, new, "inf")
    assert not rr[1][1][32:64].any() and rr[1][1][:32].any() and rr[1][1][64:96].any() and rr[0][1][32:64].any()
    for r in range(P):
        for k in range(len(SHARDS)):
            nan = R.is_nan(got[r][k], dtype)
            if (r, k) == (0, 1):
                assert nan[32:64].all() and nan.sum() == 32 and (got[r][k][32:64] == R.QNAN[dtype]).all()
            else:
                assert not nan.any(), (r, k)


def test_nothing_to_do(dev):
    cs = TG.comms(2)
    none = [[None], [None]]
    rc, st = pico_amd.loopback_mx_reduce_scatter_multi_ef(cs, none, none, none, "e4m3", sdtype="float", rdtype="float",
                                                          shard_counts=[0])
    assert rc == 0 and st == [0, 0]
    rc, st = pico_amd.loopback_mx_reduce_scatter_multi_ef(cs, [[]] * 2, [[]] * 2, [[]] * 2, "e2m1", sdtype="float",
                                                          rdtype="float", shard_counts=[])
    assert rc == 0 and st == [0, 0]
