"""MX-quantized gradient reduce-scatter, host side: bine_mx_wire_bytes against
tests/mxrs_sim.py's layout, bine_plan_mx_sum against a Python restatement of the
tile rule, the launch cut and the body flag, every refusal of the entry points
and the loopback driver in the header's order, the sim's ordered sum against a
float64 sum where every float32 step is exact, and the proof that decode *
2^(S - 127) is exact in float32 -- what lets the kernel multiply and add where
the contract could as well say fma.  No GPU: every call below ends before its
first HIP call."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import fp8_sim as F
import mx_sim as M
import mxrs_sim as R
import pico_amd
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, MX_FORMATS, BineError
from test_mx import ERR_ARG, ERR_UNSUPPORTED, ptrs, refused, sizes

S = _lib.MX_SEGS_PER_LAUNCH
CODE = {**DTYPES, **EXT_DTYPES}
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TILE_BYTES = 32768        # of the destination, counted from the segment's first element
A2A = ALGOS["alltoall"]["bine"]


# ---- bine_mx_wire_bytes ------------------------------------------------------------------------

COUNT_LISTS = [[], [0], [32], [0, 32, 0], [64, 0, 96, 32], [8192, 0, 0, 32, 8224], [32] * 17, [0] * 5,
               [2 ** 31 - 32, 32, 2 ** 31 - 32]]


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_wire_bytes_is_the_sim(fmt):
    for counts in COUNT_LISTS:
        doff, soff, D, B = R.layout(counts, fmt)
        assert pico_amd.mx_wire_bytes(counts, fmt) == (D, B), counts
        assert B % 16 == 0 and 0 <= B - (D + sum(c // 32 for c in counts)) < 16
        assert all(o % 16 == 0 for o in doff)                # every tensor's data on a 16-B boundary of the block
        assert D == sum(pico_amd.mx_dbytes(c, fmt) for c in counts)
    # 1 + 1/32 bytes per element, or 1/2 + 1/32
    assert pico_amd.mx_wire_bytes([1 << 20], fmt)[1] == (1 << 20) * (16 if fmt == "e2m1" else 32) // 32 + (1 << 15)


def test_wire_bytes_refusals():
    L = pico_amd.lib()
    d, b = ctypes.c_size_t(7), ctypes.c_size_t(7)
    ok = sizes(32, 64)
    call = lambda n, c, fmt=0, pd=ctypes.byref(d), pb=ctypes.byref(b): L.bine_mx_wire_bytes(n, c, fmt, pd, pb)  # noqa: E731
    assert call(2, ok) == 0 and (d.value, b.value) == (96, 112)
    assert call(0, None) == 0 and (d.value, b.value) == (0, 0)
    for fmt in (-1, 3, 9):
        assert call(2, ok, fmt) == ERR_ARG
    assert call(2, ok, pd=None) == ERR_ARG and call(2, ok, pb=None) == ERR_ARG
    assert call(-1, ok) == ERR_ARG and call(2, None) == ERR_ARG
    for bad in (1, 31, 33, 48, 2 ** 40 + 16):
        assert call(2, sizes(32, bad)) == ERR_ARG
    top = 2 ** 64 - 32
    assert call(2, sizes(top, 32)) == ERR_ARG                       # the data bytes' sum wraps
    assert call(1, sizes(top)) == ERR_ARG                           # data + scale bytes wrap
    assert call(1, sizes(top), 2) == 0 and d.value == top // 2      # e2m1: half the bytes, no wrap
    assert call(2, sizes(top, top), 2) == ERR_ARG
    with pytest.raises(BineError):
        pico_amd.mx_wire_bytes([33], "e4m3")


# ---- bine_plan_mx_sum --------------------------------------------------------------------------

def want_plan(dst, counts, esz):
    """one workgroup per 32 KiB of dst counted from the first element (whole blocks),
    at most S descriptors per launch, body 0 (vector) where dst is 16-B aligned"""
    recs, slot, launch, wg = [], 0, 0, 0
    for k, c in enumerate(counts):
        if c == 0:
            continue
        if slot == S:
            slot, launch, wg = 0, launch + 1, 0
        t = -(-c * esz // TILE_BYTES)
        recs.append((launch, k, wg, t, 0 if dst[k] % 16 == 0 else 1))
        slot, wg = slot + 1, wg + t
    return recs


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", sorted(ESZ))
def test_plan_mx_sum_tiles_and_body(dtype, fmt):
    esz = ESZ[dtype]
    tile = TILE_BYTES // esz
    counts = [0, 32, 64, tile - 32, tile, tile + 32, 2 * tile + 32]
    for phase in range(16 // esz):
        dst = [0x10000000 + 0x100000 * k + esz * phase for k in range(len(counts))]
        got = pico_amd.plan_mx_sum(dst, counts, dtype, fmt)
        assert got == want_plan(dst, counts, esz), phase
        assert [r[3] for r in got] == [1, 1, 1, 1, 2, 3]
        assert {r[4] for r in got} == ({0} if phase == 0 else {1})


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 37, _lib.MULTI_MAX])
def test_plan_mx_sum_launch_cut(n):
    rng = np.random.default_rng(n)
    for dtype, esz in ESZ.items():
        counts = [0 if rng.integers(4) == 0 else 32 * int(rng.integers(1, 1200)) for _ in range(n)]
        dst, a = [], 0x1000000
        for c in counts:
            null = c == 0 and rng.integers(2) == 1          # an empty tensor may be NULL
            dst.append(0 if null else 0x100000000 + a + esz * int(rng.integers(2)) * int(rng.integers(16 // esz)))
            a += (c * 4 + 64) & ~15
        got = pico_amd.plan_mx_sum(dst, counts, dtype, "e5m2")
        assert got == want_plan(dst, counts, esz)
        assert len({r[0] for r in got}) == -(-len(got) // S)


def test_plan_mx_sum_refusals():
    L = pico_amd.lib()
    a, c = (ctypes.c_uint64 * 2)(0x1000, 0x2000), (ctypes.c_size_t * 2)(32, 64)
    big = _lib.MULTI_MAX + 1
    A, C = (ctypes.c_uint64 * big)(*([0x1000] * big)), (ctypes.c_size_t * big)(*([32] * big))
    plan = lambda n, d, cnt, dt=CODE["float"], fmt=0: L.bine_plan_mx_sum(n, d, cnt, dt, fmt, None, 0)  # noqa: E731
    assert plan(2, a, c) == 2 and plan(0, None, None) == 0
    assert plan(big, A, C) == -ERR_ARG and plan(big - 1, A, C) == big - 1
    assert plan(-1, a, c) == -ERR_ARG and plan(1, None, c) == -ERR_ARG and plan(1, a, None) == -ERR_ARG
    for dt in list(range(-1, 18)) + [31, 34]:
        assert plan(1, a, c, dt) == (1 if dt == CODE["float"] else -ERR_ARG)
    for fmt in range(-1, 5):
        assert plan(1, a, c, fmt=fmt) == (1 if fmt in (0, 1, 2) else -ERR_ARG)
    zero, odd = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(0x1002)
    assert plan(1, zero, sizes(32)) == -ERR_ARG and plan(1, zero, sizes(0)) == 0
    assert plan(1, odd, sizes(32)) == -ERR_ARG and plan(1, odd, sizes(32), CODE["bfloat16"]) == 1
    for bad in (1, 31, 33, 48):
        assert plan(1, a, sizes(bad)) == -ERR_ARG
    assert plan(1, a, sizes(1 << 57)) == -ERR_ARG


# ---- the refusals of the entry points, in the header's order -------------------------------------

def test_mx_sum_segments_refusals():
    L, fn = pico_amd.lib(), "bine_mx_sum_segments"

    def call(n=1, ns=2, packed=0x9000, B=48, dst=ptrs(0x1000), c=sizes(32), dt=CODE["float"], fmt=0):
        return L.bine_mx_sum_segments(n, ns, packed, B, dst, c, dt, fmt, 1.0, None)

    for dt in (CODE["double"], CODE["uint8"], -1, 34):
        assert "ddtype" in refused(call(dt=dt), ERR_ARG, fn)
        assert "ddtype" in refused(call(n=-1, dst=None, c=None, dt=dt), ERR_ARG, fn)        # the dtype comes first
    for fmt in (-1, 3):
        assert "fmt" in refused(call(fmt=fmt), ERR_ARG, fn)
        assert "fmt" in refused(call(n=-1, fmt=fmt), ERR_ARG, fn)
    refused(call(n=-1), ERR_ARG, fn)
    refused(call(n=_lib.MULTI_MAX + 1), ERR_ARG, fn)
    assert "NULL array" in refused(call(dst=None), ERR_ARG, fn)
    assert "NULL array" in refused(call(c=None), ERR_ARG, fn)
    assert "NULL array" in refused(call(dst=None, c=sizes(33)), ERR_ARG, fn)                 # the arrays before the buffers
    assert "NULL buffer" in refused(call(dst=ptrs(0)), ERR_ARG, fn)
    assert "aligned" in refused(call(dst=ptrs(0x1002)), ERR_ARG, fn)
    assert "aligned" in refused(call(dst=ptrs(0x1001), dt=CODE["bfloat16"]), ERR_ARG, fn)
    assert "aligned" in refused(call(dst=ptrs(0x1002), c=sizes(33)), ERR_ARG, fn)            # alignment before the count
    for bad in (1, 31, 33, 48):
        assert "multiple of 32" in refused(call(c=sizes(bad)), ERR_ARG, fn)
        assert "multiple of 32" in refused(call(c=sizes(bad), ns=0), ERR_ARG, fn)            # the count before nstreams
    for ns in (-1, 0, 17, 64):
        assert "nstreams" in refused(call(ns=ns), ERR_ARG, fn)
        assert "nstreams" in refused(call(ns=ns, packed=None), ERR_ARG, fn)                  # nstreams before packed
    assert "packed" in refused(call(packed=None), ERR_ARG, fn)
    for off in (1, 4, 8):
        assert "packed" in refused(call(packed=0x9000 + off), ERR_ARG, fn)
    assert "packed" in refused(call(packed=None, B=7), ERR_ARG, fn)                          # packed before block_bytes
    for B in (0, 32, 33, 40, 47, 49):           # D + S = 33: B = 48
        assert "block_bytes" in refused(call(B=B), ERR_ARG, fn)
    # nothing to do: succeeds before packed is looked at, with no HIP call
    assert call(n=0, dst=None, c=None, packed=None, B=0) == 0
    assert call(n=2, dst=ptrs(0, 0x1000), c=sizes(0, 0), packed=None, B=0) == 0
    with pytest.raises(BineError) as e:
        pico_amd.mx_sum_segments(0x9000, 17, 48, [0x1000], "e4m3", ddtype="float", counts=[32])
    assert fn in str(e.value)


def rs(comm, n=1, sb=ptrs(0x10000), rb=ptrs(0x20000), c=sizes(64), sdt=CODE["float"], rdt=CODE["float"], fmt=0,
       sws=0x40000, rws=0x50000, wsb=4096, a2a=A2A):
    return pico_amd.lib().bine_mx_reduce_scatter_multi(comm, a2a, n, sb, rb, c, sdt, rdt, fmt, 1.0, sws, rws, wsb, None)


def test_mx_reduce_scatter_multi_refusals():
    fn = "bine_mx_reduce_scatter_multi"
    for comm in (None,):                         # NULL stands for P = 1 until the last check
        assert "sdtype" in refused(rs(comm, sdt=CODE["double"]), ERR_ARG, fn)
        assert "rdtype" in refused(rs(comm, rdt=CODE["uint8"]), ERR_ARG, fn)
        assert "fmt" in refused(rs(comm, fmt=3), ERR_ARG, fn)
        assert "fmt" in refused(rs(comm, n=-1, fmt=3), ERR_ARG, fn)                          # fmt before n
        refused(rs(comm, n=-1), ERR_ARG, fn)
        refused(rs(comm, n=_lib.MULTI_MAX + 1), ERR_ARG, fn)
        assert "NULL array" in refused(rs(comm, sb=None), ERR_ARG, fn)
        assert "NULL array" in refused(rs(comm, rb=None), ERR_ARG, fn)
        assert "NULL array" in refused(rs(comm, c=None), ERR_ARG, fn)
        assert "NULL buffer" in refused(rs(comm, sb=ptrs(0)), ERR_ARG, fn)
        assert "NULL buffer" in refused(rs(comm, rb=ptrs(0)), ERR_ARG, fn)
        assert "NULL buffer" in refused(rs(comm, rb=ptrs(0), sb=ptrs(0x10002)), ERR_ARG, fn)  # NULL before alignment
        assert "aligned" in refused(rs(comm, sb=ptrs(0x10002)), ERR_ARG, fn)
        assert "aligned" in refused(rs(comm, rb=ptrs(0x20001), rdt=CODE["float16"]), ERR_ARG, fn)
        assert "aligned" in refused(rs(comm, sb=ptrs(0x10002), c=sizes(33)), ERR_ARG, fn)    # alignment before the count
        for bad in (1, 31, 33, 48):
            assert "multiple of 32" in refused(rs(comm, c=sizes(bad)), ERR_ARG, fn)
            assert "multiple of 32" in refused(rs(comm, c=sizes(bad), sws=None), ERR_ARG, fn)  # the count before the workspaces
        assert "INT_MAX" in refused(rs(comm, c=sizes(2 ** 31)), ERR_ARG, fn)
        assert "send_ws" in refused(rs(comm, sws=None), ERR_ARG, fn)
        assert "send_ws" in refused(rs(comm, rws=None), ERR_ARG, fn)
        assert "aligned" in refused(rs(comm, sws=0x40008), ERR_ARG, fn)
        assert "aligned" in refused(rs(comm, rws=0x50004), ERR_ARG, fn)
        assert "overlap" in refused(rs(comm, rws=0x40000), ERR_ARG, fn)
        assert "overlap" in refused(rs(comm, rws=0x40000 + 4080), ERR_ARG, fn)
        assert "overlap" in refused(rs(comm, sws=0x50000 + 4080), ERR_ARG, fn)
        assert "overlap" in refused(rs(comm, rws=0x40000, wsb=16), ERR_ARG, fn)              # the overlap before the size
        for wsb in (0, 16, 79):                  # D + S = 66: B = 80
            assert "ws_bytes" in refused(rs(comm, wsb=wsb), ERR_ARG, fn)
        assert "ws_bytes" in refused(rs(comm, wsb=79, a2a=-1), ERR_ARG, fn)                  # the workspaces before the algorithm
        for bad in (-1, 0, ALGOS["allgather"]["ring"], 81):
            assert "a2a_algo" in refused(rs(comm, a2a=bad), ERR_UNSUPPORTED, fn)
            assert "a2a_algo" in refused(rs(comm, a2a=bad, n=0, sb=None, rb=None, c=None), ERR_UNSUPPORTED, fn)
    assert "comm" in refused(rs(None, wsb=80), ERR_ARG, fn)                                  # everything else passed
    assert "comm" in refused(rs(None, n=0, sb=None, rb=None, c=None, sws=None, rws=None, wsb=0), ERR_ARG, fn)
    assert "comm" in refused(rs(None, c=sizes(0), sb=ptrs(0), rb=ptrs(0), sws=None, rws=None, wsb=0), ERR_ARG, fn)


def test_loopback_mx_reduce_scatter_multi_refusals():
    L, fn = pico_amd.lib(), "bine_loopback_run_mx_reduce_scatter_multi"
    st = (ctypes.c_int * 2)(9, 9)
    sb, rb, c = ptrs(0x10000, 0x30000), ptrs(0x20000, 0x28000), sizes(64)
    sws, rws = ptrs(0x40000, 0x60000), ptrs(0x50000, 0x70000)

    def call(sb=sb, rb=rb, c=c, fmt=2, sws=sws, rws=rws, wsb=4096, a2a=A2A, rdt=CODE["bfloat16"]):
        return L.bine_loopback_run_mx_reduce_scatter_multi(None, 2, a2a, 1, sb, rb, c, CODE["float"], rdt, fmt, 1.0,
                                                           sws, rws, wsb, st)

    refused(call(fmt=3), ERR_ARG, fn)
    assert list(st) == [ERR_ARG, ERR_ARG]
    refused(call(rdt=CODE["double"]), ERR_ARG, fn)
    refused(call(sb=ptrs(0x10000, 0x30002)), ERR_ARG, fn)          # the second rank's source
    refused(call(rb=ptrs(0x20000, 0)), ERR_ARG, fn)
    refused(call(c=sizes(33)), ERR_ARG, fn)
    refused(call(sws=None), ERR_ARG, fn)
    refused(call(rws=None), ERR_ARG, fn)
    refused(call(sws=ptrs(0x40000, 0)), ERR_ARG, fn)
    refused(call(rws=ptrs(0x50000, 0x70001)), ERR_ARG, fn)
    refused(call(rws=ptrs(0x50000, 0x60000 + 64)), ERR_ARG, fn)    # the second rank's workspaces overlap
    # e2m1: D + S = 32 + 2, B = 48; two ranks need 96 bytes each
    assert "ws_bytes" in refused(call(wsb=95), ERR_ARG, fn)
    st[0] = st[1] = 9
    refused(call(a2a=ALGOS["allgather"]["ring"]), ERR_UNSUPPORTED, fn)
    assert list(st) == [ERR_UNSUPPORTED, ERR_UNSUPPORTED]
    refused(call(a2a=-1, wsb=96), ERR_UNSUPPORTED, fn)             # 96 bytes pass: the algorithm id is what is left


def test_python_wrappers():
    assert {"mx_wire_bytes", "plan_mx_sum", "mx_sum_segments", "mx_reduce_scatter_multi",
            "loopback_mx_reduce_scatter_multi"} <= set(pico_amd.__all__)
    with pytest.raises(KeyError):
        pico_amd.mx_wire_bytes([32], "e3m4")
    with pytest.raises(ValueError):
        pico_amd.plan_mx_sum([0x1000], [32, 32], "float", "e4m3")

    class FakeComm:
        size, handle, device, stream = 4, None, 0, None

    assert pico_amd.api._mx_rs_scale("avg", None, FakeComm()) == 0.25            # op="avg": 1 / comm.size
    assert pico_amd.api._mx_rs_scale("sum", None, FakeComm()) == 1.0
    assert pico_amd.api._mx_rs_scale("sum", 0.5, FakeComm()) == 0.5
    with pytest.raises(ValueError):
        pico_amd.api._mx_rs_scale("avg", 0.5, FakeComm())
    with pytest.raises(ValueError):
        pico_amd.api._mx_rs_scale("max", None, FakeComm())


# ---- the sim itself ------------------------------------------------------------------------------

def exact_value(code, S, fmt):
    """decode(code) * 2^(S - 127) as a rational number, from the format's fields (None: NaN or infinity)"""
    if fmt == "e2m1":
        v = Fraction(M.E2M1_VALUES[code & 7]) * (-1 if code & 8 else 1)
    else:
        mb, bias = F.MB[fmt], F.BIAS[fmt]
        e, m = (code & 0x7F) >> mb, code & ((1 << mb) - 1)
        if (fmt == "e4m3" and code & 0x7F == 0x7F) or (fmt == "e5m2" and e == 31):
            return None
        v = Fraction(m, 1 << mb) * Fraction(2) ** (1 - bias) if e == 0 else (1 + Fraction(m, 1 << mb)) * Fraction(2) ** (e - bias)
        v = -v if code & 0x80 else v
    return v * Fraction(2) ** (S - 127)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_decode_times_scale_is_exact_in_float32(fmt):
    """every data code under S in {0, 1, 127, 252} and under the largest S the
    quantizer writes (the scale byte of FLT_MAX: 246 / 239 / 252): the product
    is a float32 number (so rounding it changes nothing, and fma(decode, 2^(S -
    127), acc) rounds the same sum multiply-then-add does), and the sim computes
    it.  The one exception is a scale byte placed by hand above the quantizer's
    range: at S = 252 the FP8 codes of 8 and more reach 2^128, and the product
    is the multiplication's infinity, as the header says."""
    ncodes = 16 if fmt == "e2m1" else 256
    smallest = None
    s_top = M.scale_byte(0x7F7FFFFF, fmt)
    assert s_top == {"e4m3": 246, "e5m2": 239, "e2m1": 252}[fmt]
    for S in (0, 1, 127, 252, s_top):
        codes = np.arange(ncodes, dtype=np.uint8)
        data = M.pack(np.repeat(codes, 2), fmt)                          # both nibble positions
        got = M.dequant(data, np.full(M.nblk(2 * ncodes), S, dtype=np.uint8), 2 * ncodes, fmt, "float")[::2]
        for c in range(ncodes):
            v = exact_value(c, S, fmt)
            if v is None:
                assert not np.isfinite(got[c])
                continue
            if abs(v) >= Fraction(2) ** 128:
                assert S > s_top and np.isinf(got[c]) and (got[c] > 0) == (v > 0), (fmt, c, S)
                continue
            assert Fraction(float(np.float32(float(v)))) == v, (fmt, c, S)   # a float32 number: float64 holds it, float32 too
            assert Fraction(float(got[c])) == v and (np.signbit(got[c]) == bool(c & (8 if fmt == "e2m1" else 0x80)))
            if v > 0:
                smallest = v if smallest is None else min(smallest, v)
    assert smallest == Fraction(2) ** {"e4m3": -136, "e5m2": -143, "e2m1": -128}[fmt]
    assert smallest >= Fraction(2) ** -149


def narrow_blocks(counts, fmt, P, rng):
    """P wire blocks whose values span few binades: data codes of five exponent
    fields (e2m1: every code), both signs, every fraction; scale bytes 125 .. 129;
    pad bytes 0xEE"""
    doff, soff, D, B = R.layout(counts, fmt)
    ntot, ns = sum(counts), sum(c // 32 for c in counts)
    out = []
    for _ in range(P):
        b = np.full(B, 0xEE, dtype=np.uint8)
        if fmt == "e2m1":
            b[:D] = rng.integers(0, 256, D, dtype=np.uint8)
        else:
            mb = F.MB[fmt]
            lo = F.BIAS[fmt] - 2
            b[:D] = (rng.integers(0, 2, ntot) << 7) | (rng.integers(lo, lo + 5, ntot) << mb) | rng.integers(0, 1 << mb, ntot)
        b[D:D + ns] = rng.integers(125, 130, ns, dtype=np.uint8)
        out.append(b)
    return out


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_sim_sum_is_the_float64_sum_where_float32_is_exact(fmt):
    """values of at most 4 significant bits over 5 binades, scale bytes over 5
    more: every partial sum of up to 16 of them is a multiple of the smallest
    unit below 2^(4 + 5 + 5 + 4) units -- 18 bits, a float32 number -- so the
    ordered float32 sum is the exact sum and float64 agrees bit for bit"""
    rng = np.random.default_rng(6110)
    counts = [64, 0, 2048]
    for P in (1, 2, 5, 16):
        blocks = narrow_blocks(counts, fmt, P, rng)
        got = R.sum_blocks(blocks, counts, fmt, "float", 0.25)
        per = [R.values(b, counts, fmt) for b in blocks]
        for k, c in enumerate(counts):
            want = sum(per[j][k][0].astype(np.float64) for j in range(P)) * 0.25 if c else np.zeros(0)
            bits, exact = got[k]
            assert np.isfinite(want).all() and exact.all()
            assert np.array_equal(bits.view(np.float32).astype(np.float64), want), (fmt, P, k)


def test_sim_sum_order_nan_blocks_and_rounding():
    """float32 steps in stream order; S = 0xFF anywhere kills the block; one rounding for 16-bit outputs"""
    counts = [32]
    one = np.zeros(32, dtype=np.float32)
    mk = lambda v: R.pack_block([np.full(32, v, dtype=np.float32)], "float", "e4m3")  # noqa: E731
    big, small = mk(2.0 ** 24), mk(1.0)
    # (2^24 + 1) + 1 = 2^24 in float32 steps, (1 + 1) + 2^24 = 2^24 + 2
    a = R.sum_blocks([big, small, small], counts, "e4m3", "float")[0][0].view(np.float32)
    b = R.sum_blocks([small, small, big], counts, "e4m3", "float")[0][0].view(np.float32)
    assert (a == 2.0 ** 24).all() and (b == 2.0 ** 24 + 2).all()
    one[3] = np.inf
    dead = R.pack_block([one], "float", "e4m3")
    assert dead[32] == 0xFF
    for dt in ("float", "float16", "bfloat16"):
        bits, exact = R.sum_blocks([small, dead, big], counts, "e4m3", dt)[0]
        assert (bits == R.QNAN[dt]).all() and exact.all()
    # 1 + 2^-8 is not a bfloat16: one rounding, to even
    x = R.sum_blocks([small, mk(2.0 ** -8)], counts, "e4m3", "bfloat16")[0][0]
    assert (x == 0x3F80).all()
    x = R.sum_blocks([small, mk(2.0 ** -8), mk(2.0 ** -8)], counts, "e4m3", "bfloat16", 1.5)[0][0]
    assert (x == 0x3FC2).all()                   # (1 + 2^-7) * 1.5 = 1.5 + 3 * 2^-8 -> 1.5 + 2^-6 (nearest even)


def test_sim_reduce_scatter_moves_block_j_to_rank_j():
    rng = np.random.default_rng(5)
    counts, P = [32, 0, 64], 3
    src = [[rng.standard_normal(P * c).astype(np.float32) for c in counts] for _ in range(P)]
    out, recv = R.reduce_scatter(src, counts, "float", "float", "e5m2")
    for r in range(P):
        for j in range(P):
            want = R.pack_block([src[j][k][r * c:(r + 1) * c] for k, c in enumerate(counts)], "float", "e5m2")
            assert np.array_equal(recv[r][j], want)
        for k, c in enumerate(counts):
            tot = sum(src[j][k][r * c:(r + 1) * c].astype(np.float64) for j in range(P))
            if c:
                # e5m2: 2 fraction bits, relative error 2^-3 of each block's maximum per contribution
                amax = max(np.abs(src[j][k][r * c:(r + 1) * c]).max() for j in range(P))
                assert np.abs(out[r][k][0].view(np.float32) - tot).max() <= P * amax / 4
