"""Global norm and clipping, host side: bine_plan_sumsq against a Python
restatement of the tile rule, the refusals of bine_sumsq_segments and
bine_clip_segments reached through ctypes, and the refusal order of
bine_norm_multi / bine_clip_multi and their loopback drivers with no
communicator.  No GPU: every call below ends before its first HIP call."""
import ctypes
import math

import pytest

import pico_amd
from pico_amd import _lib, api
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, BineError

ERR_ARG, ERR_UNSUPPORTED = 1, 6
S = _lib.COPY_SEGS_PER_LAUNCH
TYPES = {"float": 4, "double": 8, "float16": 2, "bfloat16": 2}
CODE = {**DTYPES, **EXT_DTYPES}
TILE_VECS = 2048          # kBlock * kScaleU 16-B vectors: 32 KiB


def counts_of(esz):
    """0, 1, one vector -1 / +0 / +1, one tile -1 / +0 / +1, 3 tiles + 21 elements"""
    vec, tile = 16 // esz, TILE_VECS * 16 // esz
    return [0, 1, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1, 3 * tile + 21]


def tiles_of(addr, count, esz):
    """the tile rule: the elements before the buffer's first 16-B boundary and
    after its last full vector go with the first workgroup; one workgroup per
    2048 vectors in between, at least one per non-empty tensor"""
    nbytes = count * esz
    if nbytes == 0:
        return 0
    head = min((16 - addr % 16) % 16, nbytes)
    nvec = (nbytes - head) // 16
    return max(1, -(-nvec // TILE_VECS))


@pytest.mark.parametrize("dtype", sorted(TYPES))
def test_plan_sumsq_is_the_tile_rule(dtype):
    esz = TYPES[dtype]
    counts = counts_of(esz)
    for phase in range(0, 16, esz):
        addrs = [0x7000000 + 0x100000 * k + phase for k in range(len(counts))]
        want = [tiles_of(a, c, esz) for a, c in zip(addrs, counts)]
        assert pico_amd.plan_sumsq(addrs, counts, dtype) == sum(want), (dtype, phase)
        for a, c, w in zip(addrs, counts, want):            # one by one, and with a NULL empty in front
            assert pico_amd.plan_sumsq([a], [c], dtype) == w, (dtype, phase, c)
            assert pico_amd.plan_sumsq([0, a], [0, c], dtype) == w
    # one element past a tile is a tail element; one vector past it is a second tile, unless the
    # buffer's phase splits that vector into a head and a tail
    tile = TILE_VECS * 16 // esz
    assert pico_amd.plan_sumsq([0x1000], [tile + 1], dtype) == 1
    assert pico_amd.plan_sumsq([0x1000], [tile + 16 // esz], dtype) == 2
    assert pico_amd.plan_sumsq([0x1000 + esz], [tile + 16 // esz], dtype) == 1
    assert pico_amd.plan_sumsq([], [], dtype) == 0
    # list lengths around a launch's 128 segments and the call's 1,024: a workgroup per small tensor
    for n in (S - 1, S, S + 1, 2 * S + 37, _lib.MULTI_MAX):
        addrs = [0x1000000 + 0x100 * k + (k % (16 // esz)) * esz for k in range(n)]
        cnt = [k % 3 for k in range(n)]
        assert pico_amd.plan_sumsq(addrs, cnt, dtype) == sum(1 for c in cnt if c)


def test_sumsq_and_clip_refusals():
    """every refusal of the header, before any HIP call (there is no GPU here)"""
    L = pico_amd.lib()
    big = _lib.MULTI_MAX + 1
    f = CODE["float"]
    pv = (ctypes.c_void_p * big)(*([0x1000] * big))
    pu = (ctypes.c_uint64 * big)(*([0x1000] * big))
    cnt = (ctypes.c_size_t * big)(*([4] * big))
    null = (ctypes.c_void_p * 1)(None)
    nullu = (ctypes.c_uint64 * 1)(0)
    zero = (ctypes.c_size_t * 1)(0)
    out, scratch, norm2 = 0x20000, 0x30000, 0x40000

    def sumsq(n, bufs, counts, dtype=f, out=out, scratch=scratch, doubles=big):
        return L.bine_sumsq_segments(n, bufs, counts, dtype, out, scratch, doubles, None)

    def clip(n, bufs, counts, dtype=f, norm2=norm2, max_norm=1.0, eps=0.0, coef=None):
        return L.bine_clip_segments(n, bufs, counts, dtype, norm2, max_norm, eps, coef, None)

    def plan(n, bufs, counts, dtype=f):
        u = None if bufs is None else nullu if bufs is null else pu if bufs is pv else bufs
        return -L.bine_plan_sumsq(n, u, counts, dtype)

    # the element type: exactly the bine_scale_valid(dtype, SUM) set
    for d in sorted(CODE.values()) + [-1, 17, 31, 34, 40]:
        ok = bool(L.bine_scale_valid(d, 0))
        assert ok == (d in [CODE[t] for t in TYPES])
        if not ok:   # ... before a bad n is looked at
            assert sumsq(-1, pv, cnt, dtype=d) == ERR_ARG and clip(-1, pv, cnt, dtype=d) == ERR_ARG
            assert sumsq(1, pv, cnt, dtype=d) == ERR_ARG and clip(1, pv, cnt, dtype=d) == ERR_ARG
            assert plan(1, pv, cnt, dtype=d) == ERR_ARG
        else:
            assert L.bine_plan_sumsq(1, pu, cnt, d) == 1
    for call in (sumsq, clip, plan):
        assert call(-1, pv, cnt) == ERR_ARG
        assert call(big, pv, cnt) == ERR_ARG
        assert call(1, None, cnt) == ERR_ARG
        assert call(1, pv, None) == ERR_ARG
        assert call(1, null, cnt) == ERR_ARG                 # a NULL buffer with a non-zero count
    # a buffer not aligned to its element size
    for t, esz in TYPES.items():
        for off in range(1, 16):
            a = 0x1000 + off
            want = ERR_ARG if off % esz else 0
            assert -min(L.bine_plan_sumsq(1, (ctypes.c_uint64 * 1)(a), cnt, CODE[t]), 0) == want, (t, off)
            if want:
                assert sumsq(1, (ctypes.c_void_p * 1)(a), cnt, dtype=CODE[t]) == ERR_ARG
                assert clip(1, (ctypes.c_void_p * 1)(a), cnt, dtype=CODE[t]) == ERR_ARG
    # out: NULL, or not 8-byte aligned
    assert sumsq(1, pv, cnt, out=None) == ERR_ARG
    assert sumsq(1, pv, cnt, out=out + 4) == ERR_ARG
    assert sumsq(0, None, None, out=None) == ERR_ARG
    # scratch: fewer doubles than bine_plan_sumsq returns, or NULL when that is not zero
    tile = TILE_VECS * 4
    three = (ctypes.c_size_t * 2)(3 * tile + 1, 5)
    p2 = (ctypes.c_void_p * 2)(0x100000, 0x900000)
    assert L.bine_plan_sumsq(2, (ctypes.c_uint64 * 2)(0x100000, 0x900000), three, f) == 4
    assert sumsq(2, p2, three, doubles=3) == ERR_ARG
    assert sumsq(2, p2, three, doubles=0) == ERR_ARG
    assert sumsq(2, p2, three, scratch=None, doubles=4) == ERR_ARG
    # clip: norm2 NULL; max_norm or eps negative or NaN
    assert clip(1, pv, cnt, norm2=None) == ERR_ARG
    assert clip(0, None, None, norm2=None) == ERR_ARG
    for bad in (-1.0, -1e-300, float("nan"), -float("inf")):
        assert clip(1, pv, cnt, max_norm=bad) == ERR_ARG
        assert clip(1, pv, cnt, eps=bad) == ERR_ARG
        assert clip(0, None, None, max_norm=bad) == ERR_ARG
    # an empty tensor's pointer may be NULL, and the plan of nothing is nothing
    assert plan(1, null, zero) == 0 and plan(0, None, None) == 0
    assert L.bine_plan_sumsq(3, (ctypes.c_uint64 * 3)(0, 0x1001, 0), (ctypes.c_size_t * 3)(0, 0, 0), f) == 0
    # the Python layer
    with pytest.raises(ValueError):
        pico_amd.plan_sumsq([0x1000], [1, 2], "float")
    with pytest.raises(ValueError):
        pico_amd.sumsq_segments([0x1000], "float", counts=[1, 2], out=out, scratch=scratch, scratch_doubles=8, stream=0)
    with pytest.raises(BineError) as ei:
        pico_amd.plan_sumsq([0x1002], [1], "float")
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.sumsq_segments([0x1000], "int32", counts=[4], out=out, scratch=scratch, scratch_doubles=8, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.sumsq_segments([0x1000], "float", counts=[4], out=out, scratch=scratch, scratch_doubles=0, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.clip_segments([0x1000], norm2, -1.0, dtype="float", counts=[4], stream=0)
    assert ei.value.status == ERR_ARG


def test_norm_and_clip_multi_refusal_order():
    """the dtype; the list checks; stats; (clip) max_norm and eps; the algorithm
    id (BINE_ERR_UNSUPPORTED); comm == NULL last -- and the loopback drivers
    refuse alike on every rank, before any thread is started"""
    L = pico_amd.lib()
    f, i32 = CODE["float"], CODE["int32"]
    ok_algo = ALGOS["allreduce"]["recursivedoubling"]
    big = _lib.MULTI_MAX + 1
    p = (ctypes.c_void_p * 1)(0x1000)
    odd = (ctypes.c_void_p * 1)(0x1002)
    null = (ctypes.c_void_p * 1)(None)
    one = (ctypes.c_size_t * 1)(4)
    zero = (ctypes.c_size_t * 1)(0)
    stats = 0x20000
    nan = float("nan")

    def tri(a):
        return None if a is None else (a._type_ * 3)(*([a[0]] * 3))

    def norm(algo, n, bufs, counts, dtype=f, stats=stats):
        rc = L.bine_norm_multi(None, algo, n, bufs, counts, dtype, stats, None)
        if n <= 1 and algo == 999:      # the driver reads nranks * n entries and one stats pointer per rank
            st = (ctypes.c_int * 3)(-1, -1, -1)
            sp = (ctypes.c_void_p * 3)(stats, stats, stats)
            assert L.bine_loopback_run_norm_multi(None, 3, algo, n, tri(bufs), tri(counts), dtype, sp, st) == rc
            assert list(st) == [rc] * 3
        return rc

    def clip(algo, n, bufs, counts, dtype=f, stats=stats, max_norm=1.0, eps=1e-6):
        rc = L.bine_clip_multi(None, algo, n, bufs, counts, dtype, max_norm, eps, stats, None)
        if n <= 1 and algo == 999:
            st = (ctypes.c_int * 3)(-1, -1, -1)
            sp = (ctypes.c_void_p * 3)(stats, stats, stats)
            assert L.bine_loopback_run_clip_multi(None, 3, algo, n, tri(bufs), tri(counts), dtype, max_norm, eps, sp,
                                                  st) == rc
            assert list(st) == [rc] * 3
        return rc

    for call in (norm, clip):
        # everything right but the communicator: the algorithm id is looked at before it
        assert call(999, 1, p, one) == ERR_UNSUPPORTED
        assert call(ok_algo, 1, p, one) == ERR_ARG                   # comm == NULL, last
        assert call(999, 0, None, None) == ERR_UNSUPPORTED
        assert call(999, 1, null, zero) == ERR_UNSUPPORTED           # an empty tensor may be NULL
        # each earlier check comes before the algorithm id
        assert call(999, 1, p, one, dtype=i32) == ERR_ARG
        assert call(999, -1, p, one, dtype=i32) == ERR_ARG
        assert call(999, -1, p, one) == ERR_ARG
        assert call(999, big, p, one) == ERR_ARG
        assert call(999, 1, None, one) == ERR_ARG
        assert call(999, 1, p, None) == ERR_ARG
        assert call(999, 1, null, one) == ERR_ARG
        assert call(999, 1, odd, one) == ERR_ARG
        assert call(999, 1, p, one, stats=None) == ERR_ARG
        assert call(999, 1, p, one, stats=stats + 4) == ERR_ARG
    for bad in (-1.0, nan):
        assert clip(999, 1, p, one, max_norm=bad) == ERR_ARG
        assert clip(999, 1, p, one, eps=bad) == ERR_ARG
    assert clip(999, 1, p, one, max_norm=0.0, eps=0.0) == ERR_UNSUPPORTED
    assert clip(999, 1, p, one, max_norm=math.inf, eps=math.inf) == ERR_UNSUPPORTED
    # 16-bit types and double are taken
    for t in TYPES:
        assert norm(999, 1, p, one, dtype=CODE[t]) == ERR_UNSUPPORTED


class FakeTensor:
    def __init__(self, numel, ptr):
        self._n, self._p, self.dtype = numel, ptr, "float"

    def numel(self):
        return self._n

    def data_ptr(self):
        return self._p


class FakeComm:
    """a NULL communicator: every call below ends before it is used"""
    handle, device, stream, size = ctypes.c_void_p(0), 0, None, 4


def test_python_resolution():
    ts = [FakeTensor(5, 0x1000), FakeTensor(0, 0), FakeTensor(7, 0x2000)]
    assert list(api._norm_counts("x", ts, None)) == [5, 0, 7]          # counts default to numel()
    assert list(api._norm_counts("x", ts, [1, 2, 3])) == [1, 2, 3]
    with pytest.raises(ValueError):
        api._norm_counts("x", ts, [1, 2])
    none = FakeComm()
    with pytest.raises(BineError) as ei:
        pico_amd.norm_multi(999, ts, "float", none, stats=0x20000, stream=0)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.norm_multi(999, ts + [FakeTensor(3, 0)], "float", none, stats=0x20000, stream=0)
    assert ei.value.status == ERR_ARG                                   # a NULL tensor with elements
    with pytest.raises(BineError) as ei:
        pico_amd.clip_multi(999, ts, "float", none, -2.0, stats=0x20000, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.clip_multi("bine_lat", ts, "float", none, 2.0, stats=0x20000, stream=0)
    assert ei.value.status == ERR_ARG                                   # comm == NULL
    # scale=False (norm_multi, then clip_segments on an empty list): max_norm and eps are refused
    # first, then norm_multi's refusals in its order
    for kw in (dict(max_norm=-2.0), dict(max_norm=float("nan")), dict(max_norm=2.0, eps=-1.0)):
        with pytest.raises(BineError) as ei:
            pico_amd.clip_multi(999, ts, "float", none, stats=0x20000, stream=0, scale=False, **kw)
        assert ei.value.status == ERR_ARG
        with pytest.raises(BineError) as ei:
            pico_amd.loopback_clip_multi([none] * 2, 999, [ts, ts], "float", kw["max_norm"], kw.get("eps", 0.0),
                                         [0x20000, 0x30000], scale=False)
        assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.clip_multi(999, ts, "float", none, 2.0, stats=0x20000, stream=0, scale=False)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.clip_multi("bine_lat", ts + [FakeTensor(3, 0)], "float", none, 2.0, stats=0x20000, stream=0,
                            scale=False)
    assert ei.value.status == ERR_ARG                                   # a NULL tensor with elements
    with pytest.raises(BineError) as ei:
        pico_amd.clip_multi("bine_lat", ts, "float", none, 2.0, stats=0x20000, stream=0, scale=False)
    assert ei.value.status == ERR_ARG                                   # comm == NULL
    with pytest.raises(ValueError):
        pico_amd.loopback_norm_multi([none] * 2, "bine_lat", [ts, ts[:2]], "float", [0x20000, 0x30000])
    with pytest.raises(ValueError):
        pico_amd.loopback_clip_multi([none] * 2, "bine_lat", [ts, ts], "float", 1.0, 0.0, [0x20000])
    n, flat, c = api._loopback_norm("x", [ts, list(reversed(ts))], [0, 0], None)
    assert n == 3 and list(c) == [5, 0, 7, 7, 0, 5]                     # per-rank counts, rank major
    for name in ("sumsq_segments", "plan_sumsq", "clip_segments", "norm_multi", "clip_multi",
                 "loopback_norm_multi", "loopback_clip_multi"):
        assert name in api.__all__ and hasattr(pico_amd, name)
