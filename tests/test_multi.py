"""Multi-buffer allreduce, host side: the segmented copy's tile table
(bine_plan_segments -- the table bine_copy_segments' launcher walks), the
(dtype, op) refusals of bine_allreduce_multi with no communicator, and the
Python layer's resolution of op="avg" and counts=None.  No GPU."""
import ctypes

import numpy as np
import pytest

import pico_amd
from pico_amd import _lib, api
from pico_amd._lib import DTYPES, EXT_DTYPES, OPS, BineError

SIZES = [0, 1, 15, 16, 17, 4095, (32 << 10) - 1, 32 << 10, (32 << 10) + 1, (1 << 20) + 3]
TILE = 2048 * 16          # kBlock * kCopyU 16-B vectors
S = _lib.COPY_SEGS_PER_LAUNCH
ERR_ARG, ERR_UNSUPPORTED = 1, 6


def random_list(rng, n):
    """n segments: sizes from SIZES, destination and source phases 0..15, laid
    out one after another in two address spaces"""
    sizes = [int(rng.choice(SIZES)) for _ in range(n)]
    dst, src, d, s = [], [], 0x10000000, 0x70000000
    for b in sizes:
        dst.append(d + int(rng.integers(0, 16)))
        src.append(s + int(rng.integers(0, 16)))
        d += (b + 64) & ~15
        s += (b + 64) & ~15
    return dst, src, sizes


def check_cover(dst, src, sizes):
    tiles = pico_amd.plan_segments(dst, src, sizes)
    seen = {}
    for launch, seg, off, nb, kind in tiles:
        assert sizes[seg] > 0 and nb > 0, (seg, off, nb)
        assert off + nb <= sizes[seg], "a tile crosses its segment's end"
        if kind == 0:
            assert (dst[seg] + off) % 16 == 0 and nb % 16 == 0 and nb <= TILE, (seg, off, nb)
        else:
            assert kind == 1 and nb < 16, (seg, off, nb)
        seen.setdefault(seg, []).append((off, nb, launch, kind))
    nonempty = [k for k, b in enumerate(sizes) if b]
    assert sorted(seen) == nonempty        # empty segments produce nothing
    for i, k in enumerate(nonempty):
        cover = np.zeros(sizes[k], dtype=np.uint8)
        for off, nb, launch, _ in seen[k]:
            cover[off:off + nb] += 1
            assert launch == i // S, (k, launch, i)   # a new launch exactly every S non-empty segments
        assert (cover == 1).all(), k
        # the head ends at the destination's first 16-B boundary, the tail starts after its last full vector
        head = min((16 - dst[k] % 16) % 16, sizes[k])
        nvec = (sizes[k] - head) // 16
        small = sorted((off, nb) for off, nb, _, kind in seen[k] if kind == 1)
        want = ([(0, head)] if head else []) + \
            ([(head + 16 * nvec, sizes[k] - head - 16 * nvec)] if sizes[k] - head - 16 * nvec else [])
        assert small == want, (k, small, want)
    return tiles


def test_plan_segments_cover_random_lists():
    rng = np.random.default_rng(20240)
    for n in (1, 2, 7, 40, S - 1, S, S + 1, 3 * S + 5):
        check_cover(*random_list(rng, n))


@pytest.mark.parametrize("size", [17, 4095, (32 << 10) + 1])
def test_plan_segments_every_phase_pair(size):
    dst = [0x1000000 + 0x100000 * (16 * dp + sp) + dp for dp in range(16) for sp in range(16)]
    src = [0x9000000 + 0x100000 * (16 * dp + sp) + sp for dp in range(16) for sp in range(16)]
    tiles = check_cover(dst, src, [size] * 256)
    # the source phase does not enter the table: a segment's tiles depend on its destination alone
    per = {}
    for launch, seg, off, nb, kind in tiles:
        per.setdefault(seg, []).append((off, nb, kind))
    for dp in range(16):
        assert all(per[16 * dp + sp] == per[16 * dp] for sp in range(16))


def test_plan_segments_limits_and_empties():
    n = _lib.MULTI_MAX
    dst = [0x1000 + 64 * k for k in range(n + 1)]
    src = [0x900000 + 64 * k for k in range(n + 1)]
    tiles = pico_amd.plan_segments(dst[:n], src[:n], [16] * n)
    assert len(tiles) == n and {t[0] for t in tiles} == set(range(n // S))
    with pytest.raises(BineError) as ei:
        pico_amd.plan_segments(dst, src, [16] * (n + 1))
    assert ei.value.status == ERR_ARG
    assert pico_amd.plan_segments([], [], []) == []
    assert pico_amd.plan_segments([0, 0x1000, 0], [0, 0, 0], [0, 0, 0]) == []   # empty: pointers may be NULL
    for d, s in ((0, 0x2000), (0x1000, 0)):
        with pytest.raises(BineError) as ei:
            pico_amd.plan_segments([d], [s], [1])
        assert ei.value.status == ERR_ARG
    L = pico_amd.lib()
    assert L.bine_plan_segments(-1, None, None, None, None, 0) == -ERR_ARG
    assert L.bine_plan_segments(1, None, None, None, None, 0) == -ERR_ARG
    # empty segments do not count towards a launch's S
    sizes = [16 if k % 2 else 0 for k in range(2 * S + 2)]
    tiles = pico_amd.plan_segments(dst[:len(sizes)], src[:len(sizes)], sizes)
    assert [t[0] for t in tiles] == [0] * S + [1]


def test_refusals_without_a_communicator():
    """the (dtype, op) check comes before everything else: with comm = NULL and an
    algorithm id outside the allreduce range a pair the family accepts gets as
    far as BINE_ERR_UNSUPPORTED, a pair it refuses is BINE_ERR_ARG -- for every
    dtype and op id the dispatch-matrix test walks, in the three families"""
    L = pico_amd.lib()
    codes = sorted({**DTYPES, **EXT_DTYPES}.values()) + [-1, 17, 31, 34, 40]
    families = [(0, 1.0, L.bine_op_valid), (0, 1.0 / 3, L.bine_scale_valid), (1, 1.0, L.bine_wide_valid),
                (1, 0.25, L.bine_wide_valid)]
    n_ok = 0
    for wide, scale, valid in families:
        for d in codes:
            for o in range(-1, len(OPS) + 1):
                rc = L.bine_allreduce_multi(None, 999, 0, None, None, None, d, o, scale, wide, 0, None)
                want = ERR_UNSUPPORTED if valid(d, o) else ERR_ARG
                assert rc == want, (wide, scale, d, o, rc)
                n_ok += want == ERR_UNSUPPORTED
                st = (ctypes.c_int * 2)(-1, -1)
                rc = L.bine_loopback_run_allreduce_multi(None, 2, 999, 0, None, None, None, d, o, scale, wide, 0, st)
                assert rc == want and list(st) == [want] * 2
    assert n_ok > 100     # the three predicates were not all zero
    # then the argument checks, still before `comm`, in the header's order
    f, s = DTYPES["float"], OPS["sum"]
    one = (ctypes.c_size_t * 1)(4)
    p = (ctypes.c_void_p * 1)(0x1000)
    null = (ctypes.c_void_p * 1)(None)
    assert L.bine_allreduce_multi(None, 999, -1, None, p, one, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, _lib.MULTI_MAX + 1, None, p, one, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, 1, None, p, None, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, 1, None, None, one, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, 1, None, null, one, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, 1, null, p, one, f, s, 1.0, 0, 0, None) == ERR_ARG
    assert L.bine_allreduce_multi(None, 999, 1, None, p, one, f, s, 1.0, 0, 0, None) == ERR_UNSUPPORTED
    assert L.bine_allreduce_multi(None, 5, 1, None, p, one, f, s, 1.0, 0, 0, None) == ERR_ARG   # comm == NULL


class FakeTensor:
    def __init__(self, numel, ptr):
        self._n, self._p, self.dtype = numel, ptr, "float"

    def numel(self):
        return self._n

    def data_ptr(self):
        return self._p


def test_python_resolution():
    none = pico_amd.Comm(0, "loopback")   # a NULL communicator: every call below ends before it is used
    bufs = [FakeTensor(5, 0x1000), FakeTensor(0, 0), FakeTensor(7, 0x2000)]
    with pytest.raises(ValueError):
        pico_amd.allreduce_multi("bine_lat", None, bufs, "float", "avg", none, scale=0.5, stream=0)
    with pytest.raises(ValueError):
        pico_amd.loopback_allreduce_multi([none], "bine_lat", None, [bufs], "float", "avg", scale=0.5)
    # counts=None reads numel()
    assert list(api._multi_counts(bufs, None)) == [5, 0, 7]
    assert list(api._multi_counts(bufs, [1, 2, 3])) == [1, 2, 3]
    with pytest.raises(ValueError):
        api._multi_counts(bufs, [1, 2])
    # ... through the call: a NULL buffer is refused exactly when its numel() is not zero
    with pytest.raises(BineError) as ei:
        pico_amd.allreduce_multi(999, None, bufs, "float", "sum", none, stream=0)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(BineError) as ei:
        pico_amd.allreduce_multi(999, None, bufs + [FakeTensor(3, 0)], "float", "sum", none, stream=0)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:   # ... and explicit counts replace numel()
        pico_amd.allreduce_multi(999, None, bufs + [FakeTensor(3, 0)], "float", "sum", none, stream=0,
                                 counts=[5, 0, 7, 0])
    assert ei.value.status == ERR_UNSUPPORTED
    # wide / scaled families are chosen from the arguments: int32 has no scaled form
    with pytest.raises(BineError) as ei:
        pico_amd.allreduce_multi(999, None, bufs, "int32", "sum", none, stream=0, scale=0.5)
    assert ei.value.status == ERR_ARG
    with pytest.raises(BineError) as ei:
        pico_amd.allreduce_multi(999, None, bufs, "float", "sum", none, stream=0, wide=True)
    assert ei.value.status == ERR_ARG
    for name in ("copy_segments", "plan_segments", "allreduce_multi", "loopback_allreduce_multi"):
        assert name in api.__all__ and hasattr(pico_amd, name)
