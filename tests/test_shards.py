"""Sharded multi-buffer forms, host side: the sharded copy's tile table
(bine_plan_shards -- the table bine_copy_shards' launcher walks), the refusals of
bine_copy_shards, bine_reduce_scatter_multi and bine_allgather_multi with no
communicator and no GPU, and the Python layer's resolution of op="avg" and
shard_counts=None.  No GPU."""
import ctypes

import numpy as np
import pytest

import pico_amd
from pico_amd import _lib, api
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, OPS, BineError

SIZES = [0, 1, 15, 16, 17, 4095, (32 << 10) - 1, 32 << 10, (32 << 10) + 1, (1 << 18) + 3]
TILE = 2048 * 16          # kBlock * kCopyU 16-B vectors
S = _lib.COPY_SEGS_PER_LAUNCH
ERR_ARG, ERR_UNSUPPORTED = 1, 6
RANKS = (1, 2, 3, 8)


def random_list(rng, n, P):
    """n tensors: shard sizes from SIZES, flat phases 0..15, laid out one after
    another; a packed base of random phase"""
    sizes = [int(rng.choice(SIZES)) for _ in range(n)]
    flat, f = [], 0x70000000
    for b in sizes:
        flat.append(f + int(rng.integers(0, 16)))
        f += (P * b + 64) & ~15
    return 0x10000000 + int(rng.integers(0, 16)), flat, sizes


def check_cover(packed, flat, sizes, P, dir):
    """reads the plan only: every byte of every shard in exactly one tile, vector
    tiles on the destination's 16-B boundaries -- the destination being where the
    header puts shard j: packed + j * block_bytes + prefix sum, or flat + j * bytes"""
    tiles = pico_amd.plan_shards(packed, flat, sizes, P, dir)
    block = sum(sizes)
    poff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    seen = {}
    for launch, ten, shard, off, nb, kind in tiles:
        assert sizes[ten] > 0 and nb > 0 and 0 <= shard < P, (ten, shard, off, nb)
        assert off + nb <= sizes[ten], "a tile crosses its shard's end"
        dst = flat[ten] + shard * sizes[ten] if dir else packed + shard * block + int(poff[ten])
        if kind == 0:
            assert (dst + off) % 16 == 0 and nb % 16 == 0 and nb <= TILE, (ten, shard, off, nb)
        else:
            assert kind == 1 and nb < 16, (ten, shard, off, nb)
        seen.setdefault((ten, shard), []).append((off, nb, launch, kind, dst))
    nonempty = [k for k, b in enumerate(sizes) if b]
    assert sorted(seen) == [(k, j) for k in nonempty for j in range(P)]    # empty tensors produce nothing
    for i, k in enumerate(nonempty):
        for j in range(P):
            cover = np.zeros(sizes[k], dtype=np.uint8)
            for off, nb, launch, _, dst in seen[(k, j)]:
                cover[off:off + nb] += 1
                assert launch == i // S, (k, launch, i)   # a new launch exactly every S non-empty tensors
            assert (cover == 1).all(), (k, j)
            # the head ends at the destination's first 16-B boundary, the tail starts after its last full vector
            head = min((16 - dst % 16) % 16, sizes[k])
            nvec = (sizes[k] - head) // 16
            small = sorted((off, nb) for off, nb, _, kind, _ in seen[(k, j)] if kind == 1)
            rest = sizes[k] - head - 16 * nvec
            want = ([(0, head)] if head else []) + ([(head + 16 * nvec, rest)] if rest else [])
            assert small == want, (k, j, small, want)
    return tiles


@pytest.mark.parametrize("dir", [0, 1])
@pytest.mark.parametrize("P", RANKS)
def test_plan_shards_cover_random_lists(P, dir):
    rng = np.random.default_rng(20241 + 2 * P + dir)
    for n in (1, 2, 7, 40, S - 1, S + 1):
        check_cover(*random_list(rng, n, P), P, dir)


@pytest.mark.parametrize("dir", [0, 1])
@pytest.mark.parametrize("size", [17, 4095, (32 << 10) + 1])
def test_plan_shards_every_phase_pair(size, dir):
    """16 packed phases x 16 flat phases; the sizes are odd, so the phase of the
    destination also differs from shard to shard"""
    for pp in range(16):
        flat = [0x9000000 + 0x100000 * fp + fp for fp in range(16)]
        tiles = check_cover(0x1000000 + pp, flat, [size] * 16, 3, dir)
        # the source phase does not enter the table: a shard's tiles depend on its destination alone
        if dir == 0:
            assert pico_amd.plan_shards(0x1000000 + pp, [f + 5 for f in flat], [size] * 16, 3, dir) == tiles
        else:
            assert pico_amd.plan_shards(0x1000000 + (pp + 5) % 16, flat, [size] * 16, 3, dir) == tiles


def test_plan_shards_launches_and_empties():
    n = 2 * S + 37
    flat = [0x1000000 + 0x1000 * k for k in range(n)]
    for P in RANKS:
        tiles = check_cover(0x9000000, flat, [48] * n, P, 0)
        assert len(tiles) == n * P and {t[0] for t in tiles} == {0, 1, 2}     # ceil(n / 128) launches
    n = _lib.MULTI_MAX
    flat = [0x1000000 + 0x1000 * k for k in range(n + 1)]
    tiles = pico_amd.plan_shards(0x9000000, flat[:n], [16] * n, 2, 1)
    assert len(tiles) == 2 * n and {t[0] for t in tiles} == set(range(n // S))
    # empty tensors do not count towards a launch's S, and their pointers may be NULL
    sizes = [16 if k % 2 else 0 for k in range(2 * S + 2)]
    fl = [0x1000000 + 0x1000 * k if k % 2 else 0 for k in range(2 * S + 2)]
    tiles = check_cover(0x9000000, fl, sizes, 2, 0)
    assert [t[0] for t in tiles] == [0] * (2 * S) + [1] * 2
    assert pico_amd.plan_shards(0, [], [], 2, 0) == []
    assert pico_amd.plan_shards(0, [0, 0x1000, 0], [0, 0, 0], 2, 1) == []
    # the packed offsets: shard j of tensor k at j * block_bytes + prefix sum.  Sizes
    # of 8 B put every second tensor's packed range off the 16-B grid
    tiles = check_cover(0x9000000, flat[:4], [8, 24, 8, 40], 3, 0)
    kinds = {(t[1], t[2]): [] for t in tiles}
    for t in tiles:
        kinds[(t[1], t[2])].append((t[3], t[4], t[5]))
    # block = 80: shard j starts at 80 j + (0, 8, 32, 40)
    assert kinds[(0, 0)] == [(0, 8, 1)] and kinds[(1, 0)] == [(0, 8, 1), (8, 16, 0)]
    assert kinds[(2, 0)] == [(0, 8, 1)] and kinds[(3, 0)] == [(0, 8, 1), (8, 32, 0)]
    assert kinds[(1, 1)] == [(0, 8, 1), (8, 16, 0)] and kinds[(3, 2)] == [(0, 8, 1), (8, 32, 0)]
    tiles = check_cover(0x9000000, flat[:2], [24, 24], 2, 0)    # block = 48: shard 1 of tensor 0 at 48, tensor 1 at 24 / 72
    assert [(t[1], t[2], t[3], t[4], t[5]) for t in tiles] == [
        (0, 0, 0, 16, 0), (0, 0, 16, 8, 1), (0, 1, 0, 16, 0), (0, 1, 16, 8, 1),
        (1, 0, 0, 8, 1), (1, 0, 8, 16, 0), (1, 1, 0, 8, 1), (1, 1, 8, 16, 0)]


def test_copy_shards_refusals():
    L = pico_amd.lib()
    n = _lib.MULTI_MAX
    p = (ctypes.c_uint64 * (n + 1))(*([0x1000] * (n + 1)))
    b = (ctypes.c_size_t * (n + 1))(*([16] * (n + 1)))
    pv = (ctypes.c_void_p * (n + 1))(*([0x1000] * (n + 1)))
    null = (ctypes.c_void_p * 1)(None)
    zero = (ctypes.c_size_t * 1)(0)
    for plan in (True, False):
        def call(n, P, dir, packed, flat, sizes):
            if plan:
                fl = None if flat is None else p if flat is pv else (ctypes.c_uint64 * 1)(0)
                return -L.bine_plan_shards(n, P, dir, packed, fl, sizes, None, 0)
            return L.bine_copy_shards(n, P, dir, packed, flat, sizes, None)
        assert call(-1, 2, 0, 0x100000, pv, b) == ERR_ARG
        assert call(n + 1, 2, 0, 0x100000, pv, b) == ERR_ARG
        assert call(1, 0, 0, 0x100000, pv, b) == ERR_ARG
        assert call(1, -3, 0, 0x100000, pv, b) == ERR_ARG
        assert call(1, 65, 0, 0x100000, pv, b) == ERR_ARG        # the library's peer limit: 64
        assert call(1, 2, 2, 0x100000, pv, b) == ERR_ARG
        assert call(1, 2, -1, 0x100000, pv, b) == ERR_ARG
        assert call(1, 2, 0, 0x100000, None, b) == ERR_ARG
        assert call(1, 2, 0, 0x100000, pv, None) == ERR_ARG
        assert call(1, 2, 0, 0x100000, null, b) == ERR_ARG       # a NULL tensor with a non-zero size
        assert call(1, 2, 1, 0, pv, b) == ERR_ARG                # a NULL packed base with a non-zero size
        # success without a launch (and so without a GPU): nothing to copy
        assert call(0, 2, 0, 0, None, None) == 0
        assert call(1, 2, 1, 0, null, zero) == 0
        assert call(1, 64, 1, 0, null, zero) == 0
    with pytest.raises(ValueError):
        pico_amd.copy_shards(0x1000, [0x2000], [16, 16], 2, 0, stream=0)
    with pytest.raises(ValueError):
        pico_amd.plan_shards(0x1000, [0x2000], [16, 16], 2, 0)
    with pytest.raises(BineError) as ei:
        pico_amd.plan_shards(0x1000, [0x2000], [16], 2, 7)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.copy_shards(0x1000, [0x2000], [16], 65, 0, stream=0)
    assert ei.value.status == ERR_ARG


def test_refusals_without_a_communicator():
    """the documented order, with comm = NULL throughout: the (dtype, op) pair of
    the selected family (reduce-scatter), n, the arrays, the buffers, B > INT_MAX
    (reduce-scatter), then the algorithm id (BINE_ERR_UNSUPPORTED), then comm"""
    L = pico_amd.lib()
    codes = sorted({**DTYPES, **EXT_DTYPES}.values()) + [-1, 17, 31, 34, 40]
    families = [(0, 1.0, L.bine_op_valid), (0, 1.0 / 3, L.bine_scale_valid), (1, 1.0, L.bine_wide_valid),
                (1, 0.25, L.bine_wide_valid)]
    n_ok = 0
    for wide, scale, valid in families:
        for d in codes:
            for o in range(-1, len(OPS) + 1):
                rc = L.bine_reduce_scatter_multi(None, 999, 0, None, None, None, d, o, scale, wide, None)
                want = ERR_UNSUPPORTED if valid(d, o) else ERR_ARG
                assert rc == want, (wide, scale, d, o, rc)
                n_ok += want == ERR_UNSUPPORTED
                st = (ctypes.c_int * 2)(-1, -1)
                rc = L.bine_loopback_run_reduce_scatter_multi(None, 2, 999, 0, None, None, None, d, o, scale, wide, st)
                assert rc == want and list(st) == [want] * 2
    assert n_ok > 100     # the three predicates were not all zero
    f, s, i32 = DTYPES["float"], OPS["sum"], DTYPES["int32"]
    one = (ctypes.c_size_t * 1)(4)
    p = (ctypes.c_void_p * 1)(0x1000)
    null = (ctypes.c_void_p * 1)(None)
    inplace = (ctypes.c_void_p * 1)(_lib.IN_PLACE.value)
    big = _lib.MULTI_MAX + 1
    rs_algo = ALGOS["reduce_scatter"]["ring"]
    ag_algo = ALGOS["allgather"]["ring"]

    def tri(a):
        return None if a is None else (ctypes.c_void_p * 3)(*([a[0]] * 3))

    def rs(algo, n, sb, rb, cnt, dtype=f, op=s, scale=1.0, wide=0):
        rc = L.bine_reduce_scatter_multi(None, algo, n, sb, rb, cnt, dtype, op, scale, wide, None)
        if algo == 999 and n <= 1:     # the driver refuses alike, on every rank (it reads nranks * n pointers)
            st = (ctypes.c_int * 3)(-1, -1, -1)
            assert L.bine_loopback_run_reduce_scatter_multi(None, 3, algo, n, tri(sb), tri(rb), cnt, dtype, op,
                                                            scale, wide, st) == rc and list(st) == [rc] * 3
        return rc

    def ag(algo, n, sb, rb, cnt, dtype=f):
        rc = L.bine_allgather_multi(None, algo, n, sb, rb, cnt, dtype, None)
        if algo == 999 and n <= 1:
            st = (ctypes.c_int * 3)(-1, -1, -1)
            assert L.bine_loopback_run_allgather_multi(None, 3, algo, n, tri(sb), tri(rb), cnt, dtype,
                                                       st) == rc and list(st) == [rc] * 3
        return rc

    # a refused pair comes first: before a bad n, with comm = NULL
    assert rs(999, -1, p, p, one, dtype=i32, scale=0.5) == ERR_ARG
    assert rs(rs_algo, 1, p, p, one, dtype=i32, scale=0.5) == ERR_ARG
    assert rs(rs_algo, 1, p, p, one, dtype=f, wide=1) == ERR_ARG
    # then the argument checks, still before the algorithm id and `comm`
    assert rs(999, -1, p, p, one) == ERR_ARG and ag(999, -1, p, p, one) == ERR_ARG
    assert rs(999, big, p, p, one) == ERR_ARG and ag(999, big, p, p, one) == ERR_ARG
    assert rs(999, 1, p, p, None) == ERR_ARG and ag(999, 1, p, p, None) == ERR_ARG
    assert rs(999, 1, p, None, one) == ERR_ARG and ag(999, 1, p, None, one) == ERR_ARG
    assert rs(999, 1, None, p, one) == ERR_ARG           # the reduce-scatter has no in-place form ...
    assert ag(999, 1, None, p, one) == ERR_UNSUPPORTED   # ... the allgather's sbufs may be NULL
    assert ag(999, 1, inplace, p, one) == ERR_UNSUPPORTED
    assert rs(999, 1, p, null, one) == ERR_ARG and ag(999, 1, p, null, one) == ERR_ARG
    assert rs(999, 1, null, p, one) == ERR_ARG and ag(999, 1, null, p, one) == ERR_ARG
    zero = (ctypes.c_size_t * 1)(0)
    assert rs(999, 1, null, null, zero) == ERR_UNSUPPORTED and ag(999, 1, null, null, zero) == ERR_UNSUPPORTED
    # B > INT_MAX: the reduce-scatter only (rcounts is int)
    two = (ctypes.c_size_t * 2)(1 << 30, 1 << 30)
    p2 = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    assert L.bine_reduce_scatter_multi(None, 999, 2, p2, p2, two, f, s, 1.0, 0, None) == ERR_ARG
    assert L.bine_allgather_multi(None, 999, 2, p2, p2, two, f, None) == ERR_UNSUPPORTED
    two[1] = (1 << 30) - 1       # B = INT_MAX exactly
    assert L.bine_reduce_scatter_multi(None, 999, 2, p2, p2, two, f, s, 1.0, 0, None) == ERR_UNSUPPORTED
    # the algorithm id, then comm == NULL
    assert rs(999, 1, p, p, one) == ERR_UNSUPPORTED and ag(999, 1, p, p, one) == ERR_UNSUPPORTED
    assert rs(rs_algo, 1, p, p, one) == ERR_ARG and ag(ag_algo, 1, p, p, one) == ERR_ARG
    st = (ctypes.c_int * 2)(-1, -1)
    assert L.bine_loopback_run_allgather_multi(None, 2, 999, 0, None, None, None, f, st) == ERR_UNSUPPORTED
    assert list(st) == [ERR_UNSUPPORTED] * 2
    assert L.bine_loopback_run_allgather_multi(None, 2, 999, -1, None, None, None, f, st) == ERR_ARG
    assert list(st) == [ERR_ARG] * 2


class FakeTensor:
    def __init__(self, numel, ptr):
        self._n, self._p, self.dtype = numel, ptr, "float"

    def numel(self):
        return self._n

    def data_ptr(self):
        return self._p


class FakeComm:
    """a NULL communicator of a given size: every call below ends before it is used"""
    handle, device, stream = ctypes.c_void_p(0), 0, None

    def __init__(self, size):
        self.size = size


def test_python_resolution():
    none = FakeComm(4)
    shards = [FakeTensor(5, 0x1000), FakeTensor(0, 0), FakeTensor(7, 0x2000)]
    fulls = [FakeTensor(20, 0x10000), FakeTensor(0, 0), FakeTensor(28, 0x20000)]
    # op="avg" is op="sum" with scale = 1 / comm.size: no scale of one's own
    with pytest.raises(ValueError):
        pico_amd.reduce_scatter_multi("ring", fulls, shards, "float", "avg", none, scale=0.5, stream=0)
    with pytest.raises(ValueError):
        pico_amd.loopback_reduce_scatter_multi([none], "ring", [fulls], [shards], "float", "avg", scale=0.5)
    assert api._multi_family("avg", None, False, none) == ("sum", 0.25)
    # ... it selects the scaled family: int32 has none (BINE_ERR_ARG before the bad algorithm id is looked at)
    with pytest.raises(BineError) as ei:
        pico_amd.reduce_scatter_multi(999, fulls, shards, "int32", "avg", none, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.reduce_scatter_multi(999, fulls, shards, "int32", "sum", none, stream=0)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.reduce_scatter_multi(999, fulls, shards, "float", "avg", none, stream=0)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.reduce_scatter_multi(999, fulls, shards, "float", "sum", none, stream=0, wide=True)
    assert ei.value.status == ERR_ARG
    # the default shard_counts: each rbuf's numel() (reduce-scatter), numel() // comm.size (allgather)
    assert list(api._shard_counts("x", shards, None, 1)) == [5, 0, 7]
    assert list(api._shard_counts("x", fulls, None, 4)) == [5, 0, 7]
    assert list(api._shard_counts("x", fulls, [1, 2, 3], 4)) == [1, 2, 3]
    with pytest.raises(ValueError):
        api._shard_counts("x", fulls, [1, 2], 4)
    with pytest.raises(ValueError):
        api._shard_counts("x", fulls, None, 3)          # 20 elements do not split into 3 shards
    with pytest.raises(ValueError):
        pico_amd.allgather_multi("ring", None, fulls, "float", FakeComm(3), stream=0)
    with pytest.raises(ValueError):
        pico_amd.loopback_allgather_multi([none] * 3, "ring", None, [fulls] * 3, "float")
    with pytest.raises(ValueError):
        pico_amd.allgather_multi("ring", shards[:2], fulls, "float", none, stream=0)
    with pytest.raises(ValueError):
        pico_amd.reduce_scatter_multi("ring", None, shards, "float", "sum", none, stream=0)
    with pytest.raises(ValueError):
        pico_amd.loopback_allgather_multi([none] * 2, "ring", None, [fulls, fulls[:2]], "float")
    # ... through the calls: a NULL buffer is refused exactly when its count is not zero
    with pytest.raises(BineError) as ei:
        pico_amd.allgather_multi(999, None, fulls, "float", none, stream=0)       # sbufs=None: in place
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.allgather_multi(999, None, fulls + [FakeTensor(8, 0)], "float", none, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.allgather_multi(999, None, fulls + [FakeTensor(8, 0)], "float", none, stream=0,
                                 shard_counts=[5, 0, 7, 0])
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.reduce_scatter_multi(999, fulls + [FakeTensor(0, 0)], shards + [FakeTensor(3, 0)], "float", "sum",
                                      none, stream=0)
    assert ei.value.status == ERR_ARG
    for name in ("copy_shards", "plan_shards", "reduce_scatter_multi", "allgather_multi",
                 "loopback_reduce_scatter_multi", "loopback_allgather_multi"):
        assert name in api.__all__ and hasattr(pico_amd, name)
