"""FP8 quantization, host side: bine_fp8_scale_host against tests/fp8_sim.py's
frexp statement, bine_plan_quant against a Python restatement of the tile rule,
the launch cut and the body flag, and every refusal of the six entry points and
the loopback driver reached through ctypes.  No GPU: every call below ends
before its first HIP call."""
import ctypes

import numpy as np
import pytest

import fp8_sim as F
import pico_amd
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, FP8_FORMATS, BineError

ERR_ARG, ERR_UNSUPPORTED = 1, 6
S = _lib.COPY_SEGS_PER_LAUNCH
CODE = {**DTYPES, **EXT_DTYPES}
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TILE_VECS = 2048          # kBlock * kScaleU 16-B vectors of the wide side
RD, AG = ALGOS["allreduce"]["recursivedoubling"], ALGOS["allgather"]["ring"]


# ---- bine_fp8_scale_host ---------------------------------------------------------------------

def host(bits, fmt):
    s, i = pico_amd.fp8_scale_host(bits, fmt)
    return np.float32(s), np.float32(i)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_scale_host_boundaries(fmt):
    for bits in F.boundary_patterns(fmt):
        got, want = host(bits, fmt), F.scale_rule(bits, fmt)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (hex(bits), got, want)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_scale_host_random_patterns(fmt):
    rng = np.random.default_rng(950)
    pats = rng.integers(0, 1 << 32, 100_000, dtype=np.uint64)
    pats[::2] &= 0x7FFFFFFF                      # half of them are what bine_amax_segments can give
    L = pico_amd.lib()
    s, i = ctypes.c_float(), ctypes.c_float()
    for bits in pats.tolist():
        assert L.bine_fp8_scale_host(bits, FP8_FORMATS[fmt], ctypes.byref(s), ctypes.byref(i)) == 0
        e = F.scale_exp(bits, fmt)
        assert s.value == 2.0 ** e and i.value == 2.0 ** -e, hex(bits)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_scale_host_fills_the_format(fmt):
    """amax * scale <= FMAX < amax * 2 * scale for every finite non-zero amax, unless e was clamped"""
    rng = np.random.default_rng(951)
    pats = sorted(set(F.boundary_patterns(fmt)) | set(rng.integers(1, 0x7F800000, 20_000).tolist()))
    for bits in pats:
        if bits == 0 or bits >= 0x7F800000:
            assert host(bits, fmt) == (1.0, 1.0)
            continue
        s, i = host(bits, fmt)
        assert float(s) * float(i) == 1.0
        a = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
        if 2.0 ** -126 < float(s) < 2.0 ** 126:
            assert a * float(s) <= F.FMAX[fmt] < a * 2 * float(s), hex(bits)
        else:
            assert float(s) in (2.0 ** -126, 2.0 ** 126)


def test_scale_host_refusals():
    L = pico_amd.lib()
    s, i = ctypes.c_float(), ctypes.c_float()
    assert L.bine_fp8_scale_host(1, 0, ctypes.byref(s), ctypes.byref(i)) == 0
    for fmt in (-1, 2, 7):
        assert L.bine_fp8_scale_host(1, fmt, ctypes.byref(s), ctypes.byref(i)) == ERR_ARG
    assert L.bine_fp8_scale_host(1, 0, None, ctypes.byref(i)) == ERR_ARG
    assert L.bine_fp8_scale_host(1, 0, ctypes.byref(s), None) == ERR_ARG


# ---- bine_plan_quant -------------------------------------------------------------------------

def tiles_of(addr, count, esz):
    """the tile rule over the wide side: the elements before its first 16-B
    boundary and after its last full vector go with the first workgroup; one
    workgroup per 2,048 vectors in between, at least one per non-empty tensor"""
    if count == 0:
        return 0
    head = min(((16 - addr % 16) % 16) // esz, count)
    return max(1, -(-((count - head) * esz // 16) // TILE_VECS))


def body_of(wide, b8, esz):
    """0 (vector) when the byte side stands on a boundary of the 16 / esz bytes
    one wide vector yields where the wide side stands on a 16-B one, else 1"""
    h = ((16 - wide % 16) % 16) // esz
    return 0 if (b8 + h) % (16 // esz) == 0 else 1


def want_plan(wide, b8, counts, esz):
    recs, slot, launch, wg = [], 0, 0, 0
    for k, c in enumerate(counts):
        if c == 0:
            continue
        if slot == S:
            slot, launch, wg = 0, launch + 1, 0
        t = tiles_of(wide[k], c, esz)
        recs.append((launch, k, wg, t, body_of(wide[k], b8[k], esz)))
        slot, wg = slot + 1, wg + t
    return recs


@pytest.mark.parametrize("dtype", sorted(ESZ))
def test_plan_quant_tiles_and_body(dtype):
    esz = ESZ[dtype]
    v, tile = 16 // esz, TILE_VECS * 16 // esz
    counts = [0, 1, v - 1, v, v + 1, tile - 1, tile, tile + 1, 3 * tile + 21]
    n = len(counts)
    for sphase in range(v):                       # every element phase of the source
        for dphase in range(2 * v):               # every byte phase of the destination, twice round
            wide = [0x10000000 + 0x100000 * k + esz * sphase for k in range(n)]
            b8 = [0x50000000 + 0x100000 * k + dphase for k in range(n)]
            got = pico_amd.plan_quant(wide, b8, counts, dtype)
            assert got == want_plan(wide, b8, counts, esz), (sphase, dphase)
            h = (v - sphase) % v
            assert all(r[4] == (0 if (dphase + h) % v == 0 else 1) for r in got)


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 37, _lib.MULTI_MAX])
def test_plan_quant_launch_cut(n):
    rng = np.random.default_rng(n)
    for dtype, esz in ESZ.items():
        counts = [0 if rng.integers(4) == 0 else int(rng.integers(1, 40000)) for _ in range(n)]
        wide, b8, a = [], [], 0x1000000
        for c in counts:
            null = c == 0 and rng.integers(2) == 1          # an empty tensor may be NULL
            wide.append(0 if null else 0x100000000 + a + esz * int(rng.integers(16 // esz)))
            b8.append(0 if null else 0x500000000 + a + int(rng.integers(16)))
            a += (c * 4 + 64) & ~15
        got = pico_amd.plan_quant(wide, b8, counts, dtype)
        assert got == want_plan(wide, b8, counts, esz)
        assert len({r[0] for r in got}) == -(-len(got) // S)


def test_plan_quant_refusals():
    L = pico_amd.lib()
    a = (ctypes.c_uint64 * 2)(0x1000, 0x2000)
    c = (ctypes.c_size_t * 2)(4, 4)
    big = _lib.MULTI_MAX + 1
    A, C = (ctypes.c_uint64 * big)(*([0x1000] * big)), (ctypes.c_size_t * big)(*([4] * big))
    plan = lambda n, w, b, cnt, dt=CODE["float"]: L.bine_plan_quant(n, w, b, cnt, dt, None, 0)  # noqa: E731
    assert plan(2, a, a, c) == 2 and plan(0, None, None, None) == 0
    assert plan(big, A, A, C) == -ERR_ARG and plan(big - 1, A, A, C) == big - 1 and plan(-1, a, a, c) == -ERR_ARG
    assert plan(1, None, a, c) == -ERR_ARG and plan(1, a, None, c) == -ERR_ARG and plan(1, a, a, None) == -ERR_ARG
    for dt in list(range(-1, 18)) + [31, 34]:
        assert plan(1, a, a, c, dt) == (1 if dt == CODE["float"] else -ERR_ARG)
    zero, odd = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(0x1002)
    one, none = (ctypes.c_size_t * 1)(1), (ctypes.c_size_t * 1)(0)
    assert plan(1, zero, a, one) == -ERR_ARG and plan(1, a, zero, one) == -ERR_ARG
    assert plan(1, zero, zero, none) == 0
    assert plan(1, odd, a, one) == -ERR_ARG and plan(1, odd, a, one, CODE["bfloat16"]) == 1
    assert plan(1, a, odd, one) == 1                        # the byte side: any alignment
    with pytest.raises(BineError):
        pico_amd.plan_quant([0x1002], [0x1000], [1], "float")


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


def ptrs(*a):
    return (ctypes.c_void_p * max(len(a), 1))(*a)


def sizes(*a):
    return (ctypes.c_size_t * max(len(a), 1))(*a)


OK_OUT = 0x7000                                   # any non-NULL 4-byte aligned address: never dereferenced here


def test_amax_segments_refusals():
    L, fn = pico_amd.lib(), "bine_amax_segments"
    call = lambda n, b, c, dt=CODE["float"], out=OK_OUT: L.bine_amax_segments(n, b, c, dt, out, None)  # noqa: E731
    for dt in (CODE["double"], CODE["int32"], -1, 34):
        refused(call(1, ptrs(0x1000), sizes(4), dt), ERR_ARG, fn)
        refused(call(-1, None, None, dt, None), ERR_ARG, fn)           # the dtype comes first
    refused(call(-1, ptrs(0x1000), sizes(4)), ERR_ARG, fn)
    refused(call(_lib.MULTI_MAX + 1, ptrs(0x1000), sizes(4)), ERR_ARG, fn)
    refused(call(1, None, sizes(4)), ERR_ARG, fn)
    refused(call(1, ptrs(0x1000), None), ERR_ARG, fn)
    refused(call(1, ptrs(0), sizes(4)), ERR_ARG, fn)
    refused(call(1, ptrs(0x1002), sizes(4)), ERR_ARG, fn)
    refused(call(1, ptrs(0x1001), sizes(4), CODE["float16"]), ERR_ARG, fn)
    refused(call(1, ptrs(0), sizes(0), out=None), ERR_ARG, fn)
    refused(call(1, ptrs(0), sizes(0), out=0x7002), ERR_ARG, fn)
    refused(call(0, None, None, out=None), ERR_ARG, fn)


def test_fp8_scales_refusals():
    L, fn = pico_amd.lib(), "bine_fp8_scales"
    call = lambda n, amax=0x7000, fmt=0, scales=0x8000: L.bine_fp8_scales(n, amax, fmt, scales, None)  # noqa: E731
    for fmt in (-1, 2):
        refused(call(1, fmt=fmt), ERR_ARG, fn)
        refused(call(-1, None, fmt, None), ERR_ARG, fn)
    refused(call(-1), ERR_ARG, fn)
    refused(call(_lib.MULTI_MAX + 1), ERR_ARG, fn)
    refused(call(1, amax=None), ERR_ARG, fn)
    refused(call(1, amax=0x7001), ERR_ARG, fn)
    refused(call(1, scales=None), ERR_ARG, fn)
    refused(call(1, scales=0x8002), ERR_ARG, fn)


@pytest.mark.parametrize("deq", [False, True])
def test_quant_segments_refusals(deq):
    L = pico_amd.lib()
    fn = "bine_dequant_segments" if deq else "bine_quant_segments"

    def call(n, wide, b8, c, dt=CODE["float"], fmt=0, scales=None):
        if deq:
            return L.bine_dequant_segments(n, b8, wide, c, dt, fmt, scales, None)
        return L.bine_quant_segments(n, wide, b8, c, dt, fmt, scales, None)

    w, b, c = ptrs(0x1000), ptrs(0x2003), sizes(4)
    for dt in (CODE["double"], CODE["uint8"], -1, 34):
        refused(call(1, w, b, c, dt), ERR_ARG, fn)
        refused(call(-1, None, None, None, dt), ERR_ARG, fn)
    for fmt in (-1, 2):
        refused(call(1, w, b, c, fmt=fmt), ERR_ARG, fn)
        refused(call(-1, None, None, None, fmt=fmt), ERR_ARG, fn)
    refused(call(-1, w, b, c), ERR_ARG, fn)
    refused(call(_lib.MULTI_MAX + 1, w, b, c), ERR_ARG, fn)
    refused(call(1, None, b, c), ERR_ARG, fn)
    refused(call(1, w, None, c), ERR_ARG, fn)
    refused(call(1, w, b, None), ERR_ARG, fn)
    refused(call(1, ptrs(0), b, c), ERR_ARG, fn)
    refused(call(1, w, ptrs(0), c), ERR_ARG, fn)
    refused(call(1, ptrs(0x1002), b, c), ERR_ARG, fn)
    refused(call(1, ptrs(0x1001), b, c, CODE["bfloat16"]), ERR_ARG, fn)
    refused(call(1, ptrs(0), ptrs(0), sizes(0), scales=0x9002), ERR_ARG, fn)


def multi(comm, n, p8, src, c, amax_algo=RD, ag_algo=AG, dt=CODE["float"], fmt=0, scales=0x9000):
    return pico_amd.lib().bine_quant_multi(comm, amax_algo, ag_algo, n, p8, src, c, dt, fmt, scales, None)


def test_quant_multi_refusals():
    fn = "bine_quant_multi"
    p8, src, c = ptrs(0x2001), ptrs(0x1000), sizes(4)
    for comm in (None, 0x1234):                   # never looked at before the last check
        refused(multi(comm, 1, p8, src, c, dt=CODE["double"]), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, c, fmt=2), ERR_ARG, fn)
        refused(multi(comm, -1, p8, src, c), ERR_ARG, fn)
        refused(multi(comm, _lib.MULTI_MAX + 1, p8, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, None, src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, None, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, None), ERR_ARG, fn)
        refused(multi(comm, 1, ptrs(0), src, c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, ptrs(0), c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, ptrs(0x1002), c), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, c, scales=None), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, c, scales=0x9001), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, sizes(2 ** 31)), ERR_ARG, fn)
        for bad in (-1, 8, AG):
            refused(multi(comm, 1, p8, src, c, amax_algo=bad), ERR_UNSUPPORTED, fn)
        for bad in (-1, RD, 47, 60):
            refused(multi(comm, 1, p8, src, c, ag_algo=bad), ERR_UNSUPPORTED, fn)
        # in the header's order: a count above INT_MAX before the algorithm ids, scales before both
        refused(multi(comm, 1, p8, src, sizes(2 ** 31), amax_algo=-1), ERR_ARG, fn)
        refused(multi(comm, 1, p8, src, sizes(2 ** 31), scales=None, ag_algo=-1), ERR_ARG, fn)
    refused(multi(None, 1, p8, src, c), ERR_ARG, fn)
    refused(multi(None, 0, None, None, None), ERR_ARG, fn)


def test_loopback_quant_multi_refusals():
    L, fn = pico_amd.lib(), "bine_loopback_run_quant_multi"
    st = (ctypes.c_int * 2)(9, 9)
    p8, src, c, sc = ptrs(0x2001, 0x3001), ptrs(0x1000, 0x4000), sizes(4), ptrs(0x9000, 0xA000)

    def call(p8=p8, src=src, c=c, sc=sc, amax_algo=RD, ag_algo=AG, fmt=0):
        return L.bine_loopback_run_quant_multi(None, 2, amax_algo, ag_algo, 1, p8, src, c, CODE["float"], fmt, sc, st)

    refused(call(fmt=3), ERR_ARG, fn)
    assert list(st) == [ERR_ARG, ERR_ARG]
    refused(call(sc=None), ERR_ARG, fn)
    refused(call(sc=ptrs(0x9000, 0)), ERR_ARG, fn)
    refused(call(src=ptrs(0x1000, 0x4002)), ERR_ARG, fn)      # the second rank's source
    refused(call(p8=ptrs(0x2001, 0)), ERR_ARG, fn)
    refused(call(amax_algo=AG), ERR_UNSUPPORTED, fn)
    assert list(st) == [ERR_UNSUPPORTED, ERR_UNSUPPORTED]
    refused(call(ag_algo=RD), ERR_UNSUPPORTED, fn)


def test_python_wrappers_raise():
    with pytest.raises(BineError) as e:
        pico_amd.quant_segments([0x1002], [0x2000], "e4m3", sdtype="float", counts=[4])
    assert "bine_quant_segments" in str(e.value)
    with pytest.raises(KeyError):
        pico_amd.quant_segments([0x1000], [0x2000], "e3m4", sdtype="float", counts=[4])
