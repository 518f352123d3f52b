"""MX quantization with an error-feedback residual, host side: the numpy
contract (tests/mxef_sim.py) against float64 on every 16-bit pattern -- the
subtraction r' = v - d is exact and bounded, so widen(x) + r = d + r' up to the
one rounding of the addition -- against tests/mx_sim.py with a zero residual,
the S = 0xFF rule, 64 carried steps; bine_plan_mx_ef against the tile rule
restated, the launch cut and the body flag; every refusal of the three entry
points and the loopback driver in the header's order.  No GPU: every call
below ends before its first HIP call."""
import ctypes

import numpy as np
import pytest

import fp8_sim as F
import mx_sim as M
import mxef_sim as E
import mxrs_sim as R
import pico_amd
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, BineError
from test_mx import ERR_ARG, ERR_UNSUPPORTED, ptrs, refused, sizes

S = _lib.MX_EF_SEGS_PER_LAUNCH
CODE = {**DTYPES, **EXT_DTYPES}
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TILE_BYTES = 32768        # of the source, counted from the segment's first element
A2A = ALGOS["alltoall"]["bine"]


def unit(S_bytes, count):
    """2^(S - 127) per element, float64"""
    return np.ldexp(1.0, np.repeat(S_bytes.astype(np.int64), M.BLOCK)[:count] - 127)


def check_exact(x, r, dtype, fmt):
    """v = d + r' exactly and |r'| <= E_fmt * 2^(S - 127) wherever S != 0xFF;
    zero data and +0.0 residuals where it is"""
    v = E.add(x, r, dtype)
    data, Sb, rn = E.quant_ef(x, r, dtype, fmt)
    n = v.size
    dead = np.repeat(Sb, M.BLOCK)[:n] == 0xFF
    d = M.dequant(data, Sb, n, fmt, "float")
    live = ~dead
    # float64 holds the sum of two float32 numbers of the same block's range exactly or not at all: compare both ways
    v64, d64, r64 = v.astype(np.float64), d.astype(np.float64), rn.astype(np.float64)
    assert np.array_equal((v64 - d64)[live], r64[live])                 # the float32 subtraction did not round ...
    assert np.array_equal((d64 + r64)[live], v64[live])                 # ... and nothing else is lost
    assert (np.abs(d64) <= 2 * np.abs(v64))[live].all() and (np.abs(r64) <= np.abs(v64))[live].all()
    assert (np.abs(r64) <= E.E_FMT[fmt] * unit(Sb, n))[live].all()
    assert not rn.view(np.uint32)[dead].any()                           # +0.0
    assert not M.unpack(data, n, fmt)[dead].any()
    assert np.isfinite(v[live]).all()
    return v, data, Sb, rn


def residuals_around(x, dtype, rng):
    """one residual per element within +-40 binades of |x| (of 1 where x is zero, inf or NaN), both signs"""
    with np.errstate(invalid="ignore"):
        w = F.widen(x, dtype).astype(np.float64)         # a signalling NaN pattern is quieted: it is not used
    base = np.where(np.isfinite(w) & (w != 0), np.abs(w), 1.0)
    with np.errstate(all="ignore"):
        r = base * np.ldexp(rng.uniform(1.0, 2.0, x.size), rng.integers(-40, 41, x.size)) * rng.choice([-1.0, 1.0], x.size)
        return r.astype(np.float32)                      # a huge one becomes inf: a dead block, as the contract says


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_sim_is_exact_on_every_16_bit_pattern(dtype, fmt):
    rng = np.random.default_rng(612)
    x = F.all16(dtype)
    seen_live = 0
    for order in (np.arange(x.size), rng.permutation(x.size)):       # neighbours share a block, then strangers do
        for _ in range(2):
            xs = x[order]
            r = residuals_around(xs, dtype, rng)
            v, _, Sb, _ = check_exact(xs, r, dtype, fmt)
            seen_live += int((Sb != 0xFF).sum())
            # where float64 adds the two exactly, v is that sum rounded once
            with np.errstate(all="ignore"):
                w = F.widen(xs, dtype).astype(np.float64)
                near = np.isfinite(w) & (w != 0) & (np.abs(np.log2(np.abs(r.astype(np.float64) / np.where(w == 0, 1, w)))) < 20)
                assert np.array_equal((w + r.astype(np.float64)).astype(np.float32)[near], v[near])
    assert seen_live > 2000
    # residuals that cancel x exactly (S = 0 blocks) and ones that leave a binary32 subnormal
    xs = x[np.isfinite(F.widen(x, dtype))]
    w = F.widen(xs, dtype)
    v, data, Sb, rn = check_exact(xs, -w, dtype, fmt)
    assert not v.any() and not Sb.any() and not data.any() and not rn.any()
    tiny = (rng.integers(1, 1 << 23, xs.size).astype(np.uint32)).view(np.float32)
    v, _, Sb, _ = check_exact(xs, (tiny - w).astype(np.float32), dtype, fmt)
    assert (Sb == 0).sum() > 100


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_sim_is_exact_on_float_sources(fmt):
    rng = np.random.default_rng(613)
    n = 1 << 16
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-140, 120, n))).astype(np.float32)
    x[::97] = M.midpoints(fmt)[np.arange(x[::97].size) % M.midpoints(fmt).size]
    x[5::1024] = rng.integers(1, 1 << 23, x[5::1024].size).astype(np.uint32).view(np.float32)   # binary32 subnormals
    for _ in range(2):
        check_exact(x, residuals_around(x, "float", rng), "float", fmt)
    # blocks of subnormals alone: S = 0, the product by 2^-127 stays exact
    sub = rng.integers(0, 1 << 23, 4096).astype(np.uint32).view(np.float32)
    _, _, Sb, _ = check_exact(sub, -sub[::-1].copy(), "float", fmt)
    assert not Sb.any()
    # the clamp: a block whose maximum is past FMAX leaves at most E_fmt units
    top = np.full(32, np.nextafter(np.float32(2.0 ** (M.EMAX[fmt] + 1)), np.float32(0)), dtype=np.float32)
    _, _, Sb, rn = check_exact(top, np.zeros(32, dtype=np.float32), "float", fmt)
    assert (np.abs(rn.astype(np.float64)) > 0.99 * E.E_FMT[fmt] * unit(Sb, 32)).all()


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", F.WIDE)
def test_zero_residual_gives_the_plain_bytes(dtype, fmt):
    rng = np.random.default_rng(614)
    if dtype == "float":
        x = np.concatenate([(rng.standard_normal(4096) * np.exp2(rng.integers(-60, 60, 4096))).astype(np.float32),
                            M.midpoints(fmt), np.array([np.inf, np.nan, 0.0, 3e38], dtype=np.float32)])
        x = x[x.view(np.uint32) != 0x80000000]
        neg0 = np.float32(-0.0)
    else:
        x = F.all16(dtype)
        x = x[x != 0x8000]
        neg0 = np.uint16(0x8000)
    data, Sb, _ = E.quant_ef(x, np.zeros(x.size, dtype=np.float32), dtype, fmt)
    want, wantS = M.quant(x, dtype, fmt)
    assert np.array_equal(data, want) and np.array_equal(Sb, wantS)
    # -0 + +0 = +0: the code of +0 where the plain quantizer keeps the sign
    z = np.full(32, neg0, dtype=F.NP_WIDE[dtype])
    z[0] = 1.0 if dtype == "float" else (0x3C00 if dtype == "float16" else 0x3F80)
    data, _, rn = E.quant_ef(z, np.zeros(32, dtype=np.float32), dtype, fmt)
    plain = M.unpack(M.quant(z, dtype, fmt)[0], 32, fmt)
    sign = 8 if fmt == "e2m1" else 0x80
    assert (plain[1:] == sign).all() and not M.unpack(data, 32, fmt)[1:].any() and not rn.view(np.uint32).any()


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_the_0xff_rule(fmt):
    rng = np.random.default_rng(615)
    n = 5 * 32
    x = rng.standard_normal(n).astype(np.float32)
    r = (rng.standard_normal(n) * 0.01).astype(np.float32)
    base = E.quant_ef(x, r, "float", fmt)
    x2, r2 = x.copy(), r.copy()
    x2[32 + 7] = -np.inf                       # block 1: an infinity in x
    r2[3 * 32 + 31] = np.nan                   # block 3: a NaN in r
    x2[4 * 32] = np.finfo(np.float32).max      # block 4: x + r overflows
    r2[4 * 32] = np.float32(2.0 ** 104)
    data, Sb, rn = E.quant_ef(x2, r2, "float", fmt)
    assert list(Sb == 0xFF) == [False, True, False, True, True]
    per = M.dbytes(32, fmt)
    for b in range(5):
        blk = slice(32 * b, 32 * b + 32)
        if Sb[b] == 0xFF:
            assert not data[per * b:per * b + per].any() and not rn[blk].view(np.uint32).any()
        else:                                  # only the affected blocks change
            assert np.array_equal(data[per * b:per * b + per], base[0][per * b:per * b + per])
            assert Sb[b] == base[1][b] and np.array_equal(rn[blk].view(np.uint32), base[2][blk].view(np.uint32))
    # FLT_MAX with a residual below half an ulp does not overflow: a live block
    _, Sb, rn = E.quant_ef(np.full(32, np.finfo(np.float32).max, dtype=np.float32),
                           np.full(32, 2.0 ** 102, dtype=np.float32), "float", fmt)
    assert Sb[0] == M.scale_byte(0x7F7FFFFF, fmt) and np.isfinite(rn).all()


def carry(x, dtype, fmt, steps):
    """`steps` calls on the same x from a zero residual: (sum of d, r_T, the rounding bound of the additions)"""
    r = np.zeros(x.size, dtype=np.float32)
    tot, slack = np.zeros(x.size), np.zeros(x.size)
    for _ in range(steps):
        v = E.add(x, r, dtype)
        data, Sb, r = E.quant_ef(x, r, dtype, fmt)
        assert (Sb != 0xFF).all()
        tot += M.dequant(data, Sb, x.size, fmt, "float").astype(np.float64)
        slack += np.spacing(np.abs(v)).astype(np.float64) / 2
    return tot, r.astype(np.float64), slack


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", F.WIDE)
def test_carried_steps_lose_only_the_additions_roundings(dtype, fmt):
    rng = np.random.default_rng(616)
    n, T = 1024, 64
    xf = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32)
    x = xf if dtype == "float" else __import__("h16_util").from_f32(xf, dtype)
    tot, rT, slack = carry(x, dtype, fmt, T)
    assert (np.abs(tot + rT - T * F.widen(x, dtype).astype(np.float64)) <= slack).all()


def test_e2m1_bias_is_removed():
    """every element at 0.3 of the block's granule (0.5 * 2^(S - 127) under a
    maximum of 4): the plain quantizer sends 0 for ever, error feedback sends
    the granule three times in ten.  0.3 * 0.5 is no binary32 number, so the
    additions x + r round and the mean of the sent values lies within |r_T| / T
    of x PLUS the additions' rounding bound sum_t ulp(v_t) / 2 / T (the bound of
    the carried-steps test above, 2^-27 per step here against |r_T| / T of
    2^-9 and more).  The strict form, within |r_T| / T alone, is asserted on
    5/16 of the granule, where every addition is exact."""
    T = 64
    x = np.full(32, np.float32(0.3 * 0.5), dtype=np.float32)
    x[0] = 4.0
    tot, rT, slack = carry(x, "float", "e2m1", T)
    mean = tot / T
    assert (np.abs(mean - x.astype(np.float64)) <= (np.abs(rT) + slack) / T).all()
    assert (slack[1:] / T < 2.0 ** -26).all()
    assert (np.abs(rT) <= E.E_FMT["e2m1"] * 1.0).all()                # S = 127
    data, Sb = M.quant(x, "float", "e2m1")
    plain = M.dequant(data, Sb, 32, "e2m1", "float").astype(np.float64)
    assert Sb[0] == 127 and not plain[1:].any()
    assert (np.abs(plain - x)[1:] > 10 * ((np.abs(rT) + slack) / T)[1:]).all()
    # 5/16 of the granule: x, every residual and every sum are multiples of 2^-6 below 4, so nothing rounds
    x[1:] = np.float32(0.3125 * 0.5)
    tot, rT, _ = carry(x, "float", "e2m1", T)
    assert np.array_equal(tot + rT, T * x.astype(np.float64))          # sum of d + r_T = T x, exactly
    assert (np.abs(tot / T - x.astype(np.float64)) <= np.abs(rT) / T).all()
    assert (np.abs(plain - x)[1:] > 10 * (np.abs(rT) / T)[1:]).all() and (np.abs(rT) <= 0.25)[1:].all()


# ---- bine_plan_mx_ef -----------------------------------------------------------------------------

def body_of(src, res, d8, esz, fmt):
    per = 16 // esz if fmt != "e2m1" else 8 // esz
    return 0 if src % 16 == 0 and res % 16 == 0 and d8 % per == 0 else 1


def want_plan(src, res, d8, counts, esz, fmt):
    recs, slot, launch, wg = [], 0, 0, 0
    for k, c in enumerate(counts):
        if c == 0:
            continue
        if slot == S:
            slot, launch, wg = 0, launch + 1, 0
        t = -(-c * esz // TILE_BYTES)
        recs.append((launch, k, wg, t, body_of(src[k], res[k], d8[k], esz, fmt)))
        slot, wg = slot + 1, wg + t
    return recs


def test_segs_per_launch_is_the_largest_that_fits():
    size = lambda n: -(-(4 + 4 * (n + 1)) // 8) * 8 + 8 * (-(-n // 64)) + 40 * n   # noqa: E731  table, bitmap, descriptors
    assert size(S) <= 4096 < size(S + 1) and S == 92


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", sorted(ESZ))
def test_plan_mx_ef_tiles_and_body(dtype, fmt):
    esz = ESZ[dtype]
    tile = TILE_BYTES // esz
    counts = [0, 1, 31, 32, 33, tile - 32, tile, tile + 37, 2 * tile + 32]
    n = len(counts)
    base = lambda a: [a + 0x100000 * k for k in range(n)]  # noqa: E731
    src, res, d8, sc = base(0x10000000), base(0x30000000), base(0x50000000), base(0x70000001)
    got = pico_amd.plan_mx_ef(src, res, d8, sc, counts, dtype, fmt)
    assert got == want_plan(src, res, d8, counts, esz, fmt)
    assert [r[3] for r in got] == [1, 1, 1, 1, 1, 1, 2, 3] and {r[4] for r in got} == {0}
    per = 16 // esz if fmt != "e2m1" else 8 // esz
    # each of the three misalignments alone selects the element body
    for which, off in (("src", esz), ("res", 4), ("res", 8), ("d8", 1), ("d8", per // 2), ("src", 16 - esz)):
        a = {"src": list(src), "res": list(res), "d8": list(d8)}
        a[which][3] += off
        got = pico_amd.plan_mx_ef(a["src"], a["res"], a["d8"], sc, counts, dtype, fmt)
        assert got == want_plan(a["src"], a["res"], a["d8"], counts, esz, fmt)
        assert [r[4] for r in got] == [0, 0, 1, 0, 0, 0, 0, 0], (which, off)


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 37, _lib.MULTI_MAX])
def test_plan_mx_ef_launch_cut(n):
    rng = np.random.default_rng(n)
    for dtype, esz in ESZ.items():
        counts = [0 if rng.integers(4) == 0 else int(rng.integers(1, 40000)) for _ in range(n)]
        src, res, d8, sc, a = [], [], [], [], 0x1000000
        for c in counts:
            null = c == 0 and rng.integers(2) == 1          # an empty tensor may be NULL
            ph = lambda m: int(rng.integers(2)) * int(rng.integers(m))  # noqa: E731
            src.append(0 if null else 0x100000000 + a + esz * ph(16 // esz))
            res.append(0 if null else 0x300000000 + a + 4 * ph(4))
            d8.append(0 if null else 0x500000000 + a + ph(8))
            sc.append(0 if null else 0x700000000 + a + ph(3))
            a += (c * 4 + 64) & ~15
        got = pico_amd.plan_mx_ef(src, res, d8, sc, counts, dtype, "e5m2")
        assert got == want_plan(src, res, d8, counts, esz, "e5m2")
        assert len({r[0] for r in got}) == -(-len(got) // S)
        if n in (S, S + 1):
            full = pico_amd.plan_mx_ef([0x1000] * n, [0x2000] * n, [0x3000] * n, [0x4000] * n, [32] * n, dtype, "e4m3")
            assert [r[0] for r in full] == [0] * S + [1] * (n - S) and full[-1][2] == (0 if n > S else S - 1)


def test_plan_mx_ef_refusals():
    L = pico_amd.lib()
    a = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    s, r, d, sc, c = a(0x1000), a(0x2000), a(0x3003), a(0x4001), sizes(33)
    plan = lambda n=1, s=s, r=r, d=d, sc=sc, c=c, dt=CODE["float"], fmt=0: L.bine_plan_mx_ef(n, s, r, d, sc, c, dt, fmt, None, 0)  # noqa: E731
    assert plan() == 1 and plan(0, None, None, None, None, None) == 0
    for dt in (CODE["double"], CODE["uint8"], -1, 34):
        assert plan(dt=dt) == -ERR_ARG
    for fmt in (-1, 3):
        assert plan(fmt=fmt) == -ERR_ARG
    big = _lib.MULTI_MAX + 1
    A, C = (ctypes.c_uint64 * big)(*([0x1000] * big)), (ctypes.c_size_t * big)(*([32] * big))
    assert plan(big, A, A, A, A, C) == -ERR_ARG and plan(big - 1, A, A, A, A, C) == big - 1
    assert plan(-1) == -ERR_ARG
    for kw in ("s", "r", "d", "sc", "c"):
        assert plan(**{kw: None}) == -ERR_ARG
        if kw != "c":
            assert plan(**{kw: a(0)}) == -ERR_ARG and plan(**{kw: a(0)}, c=sizes(0)) == 0
    assert plan(s=a(0x1002)) == -ERR_ARG and plan(s=a(0x1002), dt=CODE["bfloat16"]) == 1
    for off in (1, 2, 3):
        assert plan(r=a(0x2000 + off)) == -ERR_ARG and plan(r=a(0x2000 + off), dt=CODE["float16"]) == -ERR_ARG
    assert plan(r=a(0x2004)) == 1
    assert plan(c=sizes(1 << 57)) == -ERR_ARG


# ---- the refusals of the entry points, in the header's order --------------------------------------

def test_mx_quant_ef_segments_refusals():
    L, fn = pico_amd.lib(), "bine_mx_quant_ef_segments"

    def call(n=1, s=ptrs(0x1000), r=ptrs(0x2000), d=ptrs(0x3003), sc=ptrs(0x4001), c=sizes(33), dt=CODE["float"], fmt=0):
        return L.bine_mx_quant_ef_segments(n, s, r, d, sc, c, dt, fmt, None)

    for dt in (CODE["double"], CODE["uint8"], -1, 34):
        assert "sdtype" in refused(call(dt=dt), ERR_ARG, fn)
        assert "sdtype" in refused(call(n=-1, s=None, dt=dt, fmt=7), ERR_ARG, fn)           # the dtype comes first
    for fmt in (-1, 3):
        assert "fmt" in refused(call(fmt=fmt), ERR_ARG, fn)
        assert "fmt" in refused(call(n=-1, fmt=fmt), ERR_ARG, fn)                           # fmt before n
    refused(call(n=-1), ERR_ARG, fn)
    refused(call(n=_lib.MULTI_MAX + 1), ERR_ARG, fn)
    for kw in ("s", "r", "d", "sc", "c"):
        assert "NULL array" in refused(call(**{kw: None}), ERR_ARG, fn)
    assert "NULL array" in refused(call(r=None, s=ptrs(0)), ERR_ARG, fn)                    # the arrays before the buffers
    for kw in ("s", "r", "d", "sc"):
        assert "NULL buffer" in refused(call(**{kw: ptrs(0)}), ERR_ARG, fn)
    assert "NULL buffer" in refused(call(r=ptrs(0), s=ptrs(0x1002)), ERR_ARG, fn)           # NULL before alignment
    assert "aligned" in refused(call(s=ptrs(0x1002)), ERR_ARG, fn)
    assert "aligned" in refused(call(s=ptrs(0x1001), dt=CODE["float16"]), ERR_ARG, fn)
    for off in (1, 2, 3):
        assert "residual" in refused(call(r=ptrs(0x2000 + off), dt=CODE["bfloat16"]), ERR_ARG, fn)
    # nothing to do: succeeds with no HIP call
    assert call(n=0, s=None, r=None, d=None, sc=None, c=None) == 0
    assert call(n=2, s=ptrs(0, 0), r=ptrs(0, 0), d=ptrs(0, 0), sc=ptrs(0, 0), c=sizes(0, 0)) == 0
    with pytest.raises(BineError) as e:
        pico_amd.mx_quant_ef_segments([0x1000], [0x2001], [0x3000], [0x4000], "e4m3", sdtype="float", counts=[32])
    assert fn in str(e.value)


def rs(comm, n=1, sb=ptrs(0x10000), res=ptrs(0x80000), rb=ptrs(0x20000), c=sizes(64), sdt=CODE["float"],
       rdt=CODE["float"], fmt=0, sws=0x40000, rws=0x50000, wsb=4096, a2a=A2A):
    return pico_amd.lib().bine_mx_reduce_scatter_multi_ef(comm, a2a, n, sb, res, rb, c, sdt, rdt, fmt, 1.0, sws, rws, wsb,
                                                          None)


def test_mx_reduce_scatter_multi_ef_refusals():
    fn = "bine_mx_reduce_scatter_multi_ef"
    comm = None                                  # NULL stands for P = 1 until the last check
    assert "sdtype" in refused(rs(comm, sdt=CODE["double"]), ERR_ARG, fn)
    assert "rdtype" in refused(rs(comm, rdt=CODE["uint8"]), ERR_ARG, fn)
    assert "fmt" in refused(rs(comm, fmt=3), ERR_ARG, fn)
    assert "fmt" in refused(rs(comm, n=-1, fmt=3), ERR_ARG, fn)                              # fmt before n
    refused(rs(comm, n=-1), ERR_ARG, fn)
    refused(rs(comm, n=_lib.MULTI_MAX + 1), ERR_ARG, fn)
    for kw in ("sb", "res", "rb", "c"):
        assert "NULL array" in refused(rs(comm, **{kw: None}), ERR_ARG, fn)
    for kw in ("sb", "res", "rb"):
        assert "NULL buffer" in refused(rs(comm, **{kw: ptrs(0)}), ERR_ARG, fn)
    assert "NULL buffer" in refused(rs(comm, res=ptrs(0), sb=ptrs(0x10002)), ERR_ARG, fn)    # NULL before alignment
    assert "aligned" in refused(rs(comm, sb=ptrs(0x10002)), ERR_ARG, fn)
    assert "aligned" in refused(rs(comm, rb=ptrs(0x20001), rdt=CODE["float16"]), ERR_ARG, fn)
    for off in (1, 2):
        assert "residual" in refused(rs(comm, res=ptrs(0x80000 + off), sdt=CODE["bfloat16"]), ERR_ARG, fn)
    assert "residual" in refused(rs(comm, res=ptrs(0x80002), c=sizes(33)), ERR_ARG, fn)      # alignment before the count
    for bad in (1, 31, 33, 48):
        assert "multiple of 32" in refused(rs(comm, c=sizes(bad)), ERR_ARG, fn)
        assert "multiple of 32" in refused(rs(comm, c=sizes(bad), sws=None), ERR_ARG, fn)    # the count before the workspaces
    assert "INT_MAX" in refused(rs(comm, c=sizes(2 ** 31)), ERR_ARG, fn)
    assert "send_ws" in refused(rs(comm, sws=None), ERR_ARG, fn)
    assert "send_ws" in refused(rs(comm, rws=None), ERR_ARG, fn)
    assert "aligned" in refused(rs(comm, sws=0x40008), ERR_ARG, fn)
    assert "overlap" in refused(rs(comm, rws=0x40000 + 4080), ERR_ARG, fn)
    assert "overlap" in refused(rs(comm, rws=0x40000, wsb=16), ERR_ARG, fn)                  # the overlap before the size
    for wsb in (0, 16, 79):                      # D + S = 66: B = 80
        assert "ws_bytes" in refused(rs(comm, wsb=wsb), ERR_ARG, fn)
    assert "ws_bytes" in refused(rs(comm, wsb=79, a2a=-1), ERR_ARG, fn)                      # the workspaces before the algorithm
    for bad in (-1, 0, ALGOS["allgather"]["ring"], 81):
        assert "a2a_algo" in refused(rs(comm, a2a=bad), ERR_UNSUPPORTED, fn)
        assert "a2a_algo" in refused(rs(comm, a2a=bad, n=0, sb=None, res=None, rb=None, c=None), ERR_UNSUPPORTED, fn)
    assert "comm" in refused(rs(None, wsb=80), ERR_ARG, fn)                                  # everything else passed
    assert "comm" in refused(rs(None, n=0, sb=None, res=None, rb=None, c=None, sws=None, rws=None, wsb=0), ERR_ARG, fn)


def test_loopback_mx_reduce_scatter_multi_ef_refusals():
    L, fn = pico_amd.lib(), "bine_loopback_run_mx_reduce_scatter_multi_ef"
    st = (ctypes.c_int * 2)(9, 9)
    sb, rb, c = ptrs(0x10000, 0x30000), ptrs(0x20000, 0x28000), sizes(64)
    res = ptrs(0x80000, 0x90000)
    sws, rws = ptrs(0x40000, 0x60000), ptrs(0x50000, 0x70000)

    def call(sb=sb, res=res, rb=rb, c=c, fmt=2, sws=sws, rws=rws, wsb=4096, a2a=A2A, rdt=CODE["bfloat16"]):
        return L.bine_loopback_run_mx_reduce_scatter_multi_ef(None, 2, a2a, 1, sb, res, rb, c, CODE["float"], rdt, fmt,
                                                              1.0, sws, rws, wsb, st)

    refused(call(fmt=3), ERR_ARG, fn)
    assert list(st) == [ERR_ARG, ERR_ARG]
    refused(call(rdt=CODE["double"]), ERR_ARG, fn)
    refused(call(sb=ptrs(0x10000, 0x30002)), ERR_ARG, fn)          # the second rank's source
    refused(call(res=None), ERR_ARG, fn)
    refused(call(res=ptrs(0x80000, 0)), ERR_ARG, fn)               # the second rank's residual
    assert "residual" in refused(call(res=ptrs(0x80000, 0x90002)), ERR_ARG, fn)
    refused(call(rb=ptrs(0x20000, 0)), ERR_ARG, fn)
    refused(call(c=sizes(33)), ERR_ARG, fn)
    refused(call(sws=None), ERR_ARG, fn)
    refused(call(rws=ptrs(0x50000, 0x70001)), ERR_ARG, fn)
    refused(call(rws=ptrs(0x50000, 0x60000 + 64)), ERR_ARG, fn)    # the second rank's workspaces overlap
    assert "ws_bytes" in refused(call(wsb=95), ERR_ARG, fn)        # e2m1: B = 48; two ranks need 96 bytes each
    st[0] = st[1] = 9
    refused(call(a2a=ALGOS["allgather"]["ring"]), ERR_UNSUPPORTED, fn)
    assert list(st) == [ERR_UNSUPPORTED, ERR_UNSUPPORTED]
    refused(call(a2a=-1, wsb=96), ERR_UNSUPPORTED, fn)


def test_python_wrappers_and_sim_exchange():
    assert {"mx_quant_ef_segments", "plan_mx_ef", "mx_reduce_scatter_multi_ef",
            "loopback_mx_reduce_scatter_multi_ef"} <= set(pico_amd.__all__)
    with pytest.raises(ValueError):
        pico_amd.plan_mx_ef([0x1000], [0x2000], [0x3000], [0x4000], [32, 32], "float", "e4m3")
    with pytest.raises(ValueError):
        pico_amd.mx_quant_ef_segments([0x1000], [], [0x3000], [0x4000], "e4m3", sdtype="float", counts=[32])
    # the sim's exchange with zero residuals, no -0: the plain sim's shards; the residuals are what each rank kept
    rng = np.random.default_rng(617)
    counts, P = [32, 0, 64], 3
    src = [[rng.standard_normal(P * c).astype(np.float32) for c in counts] for _ in range(P)]
    zero = [[np.zeros(P * c, dtype=np.float32) for c in counts] for _ in range(P)]
    out, new, recv = E.reduce_scatter_ef(src, zero, counts, "float", "float", "e2m1", 0.5)
    plain, precv = R.reduce_scatter(src, counts, "float", "float", "e2m1", 0.5)
    for r in range(P):
        assert all(np.array_equal(recv[r][j], precv[r][j]) for j in range(P))
        for k, c in enumerate(counts):
            assert np.array_equal(out[r][k][0], plain[r][k][0])
            for j in range(P):
                sl = slice(j * c, (j + 1) * c)
                _, _, want = E.quant_ef(src[r][k][sl], zero[r][k][sl], "float", "e2m1")
                assert np.array_equal(new[r][k][sl], want)
