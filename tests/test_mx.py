"""MX block-scaled quantization, host side: bine_mx_scale_host against
tests/mx_sim.py's frexp statement, bine_plan_mx against a Python restatement of
the tile rule, the launch cut and the body flag, and every refusal of the entry
points and the loopback driver reached through ctypes.  No GPU: every call
below ends before its first HIP call."""
import ctypes

import numpy as np
import pytest

import mx_sim as M
import pico_amd
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, MX_FORMATS, BineError

ERR_ARG, ERR_UNSUPPORTED = 1, 6
S = _lib.MX_SEGS_PER_LAUNCH
CODE = {**DTYPES, **EXT_DTYPES}
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TILE_BYTES = 32768        # of the wide side, counted from the segment's first element
AG, RD = ALGOS["allgather"]["ring"], ALGOS["allreduce"]["recursivedoubling"]


# ---- bine_mx_scale_host ------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", M.FORMATS)
def test_scale_host_sweep(fmt):
    for bits in M.scale_patterns():
        assert pico_amd.mx_scale_host(bits, fmt) == M.scale_byte(bits, fmt), hex(bits)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_scale_host_random_patterns(fmt):
    rng = np.random.default_rng(3200)
    L, s = pico_amd.lib(), ctypes.c_uint8()
    for bits in rng.integers(0, 1 << 31, 50_000, dtype=np.uint64).tolist():
        assert L.bine_mx_scale_host(bits, MX_FORMATS[fmt], ctypes.byref(s)) == 0
        assert s.value == M.scale_byte(bits, fmt), hex(bits)


def test_scale_host_refusals():
    L, s = pico_amd.lib(), ctypes.c_uint8()
    for fmt in (0, 1, 2):
        assert L.bine_mx_scale_host(1, fmt, ctypes.byref(s)) == 0
        assert L.bine_mx_scale_host(1, fmt, None) == ERR_ARG
    for fmt in (-1, 3, 7):
        assert L.bine_mx_scale_host(1, fmt, ctypes.byref(s)) == ERR_ARG


# ---- bine_plan_mx ------------------------------------------------------------------------------

def tiles_of(count, esz):
    """one workgroup per 32 KiB of the wide side counted from the first element"""
    return -(-count * esz // TILE_BYTES)


def body_of(wide, d8, esz, fmt):
    """0 (vector) where the wide side is 16-B aligned and the data side aligned
    to the bytes one wide vector yields, else 1"""
    per = 16 // esz if fmt != "e2m1" else 8 // esz
    return 0 if wide % 16 == 0 and d8 % per == 0 else 1


def want_plan(wide, d8, counts, esz, fmt):
    recs, slot, launch, wg = [], 0, 0, 0
    for k, c in enumerate(counts):
        if c == 0:
            continue
        if slot == S:
            slot, launch, wg = 0, launch + 1, 0
        t = tiles_of(c, esz)
        recs.append((launch, k, wg, t, body_of(wide[k], d8[k], esz, fmt)))
        slot, wg = slot + 1, wg + t
    return recs


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", sorted(ESZ))
def test_plan_mx_tiles_and_body(dtype, fmt):
    esz = ESZ[dtype]
    v, tile = 16 // esz, TILE_BYTES // esz
    counts = [0, 1, 31, 32, 33, tile - 1, tile, tile + 1, 3 * tile + 21]
    n = len(counts)
    vec = 0
    for sphase in range(v):                       # every element phase of the wide side
        for dphase in range(2 * v):               # every byte phase of the data side, twice round
            wide = [0x10000000 + 0x100000 * k + esz * sphase for k in range(n)]
            d8 = [0x50000000 + 0x100000 * k + dphase for k in range(n)]
            sc = [0x70000000 + 0x100000 * k + (dphase * 7 + sphase) % 5 for k in range(n)]   # any alignment
            got = pico_amd.plan_mx(wide, d8, sc, counts, dtype, fmt)
            assert got == want_plan(wide, d8, counts, esz, fmt), (sphase, dphase)
            assert [r[3] for r in got] == [1, 1, 1, 1, 1, 1, 2, 4]
            vec += sum(1 for r in got if r[4] == 0)
    per = v if fmt != "e2m1" else v // 2
    assert vec == 8 * (2 * v // per)              # only phase 0 of the wide side, every per-th of the data side


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 37, _lib.MULTI_MAX])
def test_plan_mx_launch_cut(n):
    rng = np.random.default_rng(n)
    for dtype, esz in ESZ.items():
        for fmt in M.FORMATS:
            counts = [0 if rng.integers(4) == 0 else int(rng.integers(1, 40000)) for _ in range(n)]
            wide, d8, sc, a = [], [], [], 0x1000000
            for c in counts:
                null = c == 0 and rng.integers(2) == 1          # an empty tensor may be NULL
                wide.append(0 if null else 0x100000000 + a + esz * int(rng.integers(2)) * int(rng.integers(16 // esz)))
                d8.append(0 if null else 0x500000000 + a + int(rng.integers(2)) * int(rng.integers(16)))
                sc.append(0 if null else 0x700000000 + a + int(rng.integers(16)))
                a += (c * 4 + 64) & ~15
            got = pico_amd.plan_mx(wide, d8, sc, counts, dtype, fmt)
            assert got == want_plan(wide, d8, counts, esz, fmt)
            assert len({r[0] for r in got}) == -(-len(got) // S)


def test_plan_mx_refusals():
    L = pico_amd.lib()
    a = (ctypes.c_uint64 * 2)(0x1000, 0x2000)
    c = (ctypes.c_size_t * 2)(4, 4)
    big = _lib.MULTI_MAX + 1
    A, C = (ctypes.c_uint64 * big)(*([0x1000] * big)), (ctypes.c_size_t * big)(*([4] * big))
    plan = lambda n, w, d, s, cnt, dt=CODE["float"], fmt=0: L.bine_plan_mx(n, w, d, s, cnt, dt, fmt, None, 0)  # noqa: E731
    assert plan(2, a, a, a, c) == 2 and plan(0, None, None, None, None) == 0
    assert plan(big, A, A, A, C) == -ERR_ARG and plan(big - 1, A, A, A, C) == big - 1
    assert plan(-1, a, a, a, c) == -ERR_ARG
    assert plan(1, None, a, a, c) == -ERR_ARG and plan(1, a, None, a, c) == -ERR_ARG
    assert plan(1, a, a, None, c) == -ERR_ARG and plan(1, a, a, a, None) == -ERR_ARG
    for dt in list(range(-1, 18)) + [31, 34]:
        assert plan(1, a, a, a, c, dt) == (1 if dt == CODE["float"] else -ERR_ARG)
    for fmt in range(-1, 5):
        assert plan(1, a, a, a, c, fmt=fmt) == (1 if fmt in (0, 1, 2) else -ERR_ARG)
    zero, odd = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(0x1002)
    one, none, huge = (ctypes.c_size_t * 1)(1), (ctypes.c_size_t * 1)(0), (ctypes.c_size_t * 1)(1 << 57)
    assert plan(1, zero, a, a, one) == -ERR_ARG and plan(1, a, zero, a, one) == -ERR_ARG
    assert plan(1, a, a, zero, one) == -ERR_ARG
    assert plan(1, zero, zero, zero, none) == 0
    assert plan(1, odd, a, a, one) == -ERR_ARG and plan(1, odd, a, a, one, CODE["bfloat16"]) == 1
    assert plan(1, a, odd, odd, one) == 1                   # the byte sides: any alignment
    assert plan(1, a, a, a, huge) == -ERR_ARG
    with pytest.raises(BineError):
        pico_amd.plan_mx([0x1002], [0x1000], [0x3000], [1], "float", "e4m3")


# ---- the refusals of the entry points ------------------------------------------------------------

def refused(rc, want, fn):
    """the status, and a reason naming the call left in bine_last_error BY THIS
    call: another call's error is planted in its place afterwards, so the next
    refusal cannot pass on this one's string"""
    L = pico_amd.lib()
    assert rc == want, (fn, rc)
    err = L.bine_last_error().decode()
    assert err.startswith(fn + ":") and len(err) > len(fn) + 2, err
    assert L.bine_rccl_abi_check(22509, 22707) != 0 and b"skew" in L.bine_last_error()
    return err


def ptrs(*a):
    return (ctypes.c_void_p * max(len(a), 1))(*a)


def sizes(*a):
    return (ctypes.c_size_t * max(len(a), 1))(*a)


@pytest.mark.parametrize("deq", [False, True])
def test_mx_segments_refusals(deq):
    L = pico_amd.lib()
    fn = "bine_mx_dequant_segments" if deq else "bine_mx_quant_segments"

    def call(n, wide, d8, sc, c, dt=CODE["float"], fmt=0):
        if deq:
            return L.bine_mx_dequant_segments(n, d8, sc, wide, c, dt, fmt, None)
        return L.bine_mx_quant_segments(n, wide, d8, sc, c, dt, fmt, None)

    w, d, s, c = ptrs(0x1000), ptrs(0x2003), ptrs(0x3001), sizes(4)
    for dt in (CODE["double"], CODE["uint8"], -1, 34):
        assert "dtype" in refused(call(1, w, d, s, c, dt), ERR_ARG, fn)
        refused(call(-1, None, None, None, None, dt), ERR_ARG, fn)       # the dtype comes first
    for fmt in (-1, 3):
        assert "fmt" in refused(call(1, w, d, s, c, fmt=fmt), ERR_ARG, fn)
        assert "fmt" in refused(call(-1, None, None, None, None, fmt=fmt), ERR_ARG, fn)
    refused(call(-1, w, d, s, c), ERR_ARG, fn)
    refused(call(_lib.MULTI_MAX + 1, w, d, s, c), ERR_ARG, fn)
    refused(call(1, None, d, s, c), ERR_ARG, fn)
    refused(call(1, w, None, s, c), ERR_ARG, fn)
    refused(call(1, w, d, None, c), ERR_ARG, fn)
    refused(call(1, w, d, s, None), ERR_ARG, fn)
    assert "NULL array" in refused(call(1, None, ptrs(0), s, c), ERR_ARG, fn)    # the arrays before the buffers
    refused(call(1, ptrs(0), d, s, c), ERR_ARG, fn)
    refused(call(1, w, ptrs(0), s, c), ERR_ARG, fn)
    refused(call(1, w, d, ptrs(0), c), ERR_ARG, fn)
    refused(call(1, ptrs(0x1002), d, s, c), ERR_ARG, fn)
    refused(call(1, ptrs(0x1001), d, s, c, CODE["bfloat16"]), ERR_ARG, fn)


def multi(comm, n, p8, s8, src, c, ag_algo=AG, dt=CODE["float"], fmt=0):
    return pico_amd.lib().bine_mx_quant_multi(comm, ag_algo, n, p8, s8, src, c, dt, fmt, None)


def test_mx_quant_multi_refusals():
    fn = "bine_mx_quant_multi"
    p8, s8, src, c = ptrs(0x2001), ptrs(0x3003), ptrs(0x1000), sizes(32)
    for comm in (None, 0x1234):                   # never looked at before the last check
        assert "sdtype" in refused(multi(comm, 1, p8, s8, src, c, dt=CODE["double"]), ERR_ARG, fn)
        assert "fmt" in refused(multi(comm, 1, p8, s8, src, c, fmt=3), ERR_ARG, fn)
        refused(multi(comm, -1, p8, s8, src, c), ERR_ARG, fn)
        assert "MULTI_MAX / 2" in refused(multi(comm, _lib.MULTI_MAX // 2 + 1, p8, s8, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, None, s8, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, None, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, s8, None, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, s8, src, None), ERR_ARG, fn)
        refused(multi(comm, 1, ptrs(0), s8, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, ptrs(0), src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, s8, ptrs(0), c), ERR_ARG, fn)
        assert "aligned" in refused(multi(comm, 1, p8, s8, ptrs(0x1002), c), ERR_ARG, fn)
        for bad in (33, 1, 31, 48):
            assert "multiple of 32" in refused(multi(comm, 1, p8, s8, src, sizes(bad)), ERR_ARG, fn)
        refused(multi(comm, 1, p8, s8, src, sizes(2 ** 31)), ERR_ARG, fn)
        for bad in (-1, RD, 47, 60):
            refused(multi(comm, 1, p8, s8, src, c, ag_algo=bad), ERR_UNSUPPORTED, fn)
        # in the header's order: the source's alignment before the count, the count before the algorithm id
        assert "aligned" in refused(multi(comm, 1, p8, s8, ptrs(0x1002), sizes(33)), ERR_ARG, fn)
        refused(multi(comm, 1, p8, s8, src, sizes(33), ag_algo=-1), ERR_ARG, fn)
        assert "fmt" in refused(multi(comm, -1, None, None, None, None, fmt=3, ag_algo=-1), ERR_ARG, fn)
    assert "comm" in refused(multi(None, 1, p8, s8, src, c), ERR_ARG, fn)
    refused(multi(None, 0, None, None, None, None), ERR_ARG, fn)


def test_loopback_mx_quant_multi_refusals():
    L, fn = pico_amd.lib(), "bine_loopback_run_mx_quant_multi"
    st = (ctypes.c_int * 2)(9, 9)
    p8, s8, src, c = ptrs(0x2001, 0x3001), ptrs(0x5000, 0x6003), ptrs(0x1000, 0x4000), sizes(64)

    def call(p8=p8, s8=s8, src=src, c=c, ag_algo=AG, fmt=2):
        return L.bine_loopback_run_mx_quant_multi(None, 2, ag_algo, 1, p8, s8, src, c, CODE["float"], fmt, st)

    refused(call(fmt=3), ERR_ARG, fn)
    assert list(st) == [ERR_ARG, ERR_ARG]
    refused(call(src=ptrs(0x1000, 0x4002)), ERR_ARG, fn)      # the second rank's source
    refused(call(p8=ptrs(0x2001, 0)), ERR_ARG, fn)
    refused(call(s8=ptrs(0x5000, 0)), ERR_ARG, fn)
    refused(call(c=sizes(33)), ERR_ARG, fn)
    refused(call(ag_algo=RD), ERR_UNSUPPORTED, fn)
    assert list(st) == [ERR_UNSUPPORTED, ERR_UNSUPPORTED]


def test_python_wrappers_raise():
    with pytest.raises(BineError) as e:
        pico_amd.mx_quant_segments([0x1002], [0x2000], [0x3000], "e4m3", sdtype="float", counts=[4])
    assert "bine_mx_quant_segments" in str(e.value)
    with pytest.raises(KeyError):
        pico_amd.mx_quant_segments([0x1000], [0x2000], [0x3000], "e3m4", sdtype="float", counts=[4])
    assert pico_amd.mx_dbytes(33, "e2m1") == 17 and pico_amd.mx_dbytes(33, "e5m2") == 33
