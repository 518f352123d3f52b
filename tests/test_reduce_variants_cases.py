"""The shape table of tests/test_gpu_reduce_variants.py and
tools/reduce_env_check.py (tests/reduce_variants_cases.py) reaches what it
says -- proved on the CPU with the host model of k_reduce's index arithmetic:
for every U, every launch of the table writes each vector below nvec exactly
once and none at or past it (a); the multi-trip shape under a cap of 2 or 3
workgroups takes a second trip (b), ends a workgroup on a partial tile after
full trips (c), leaves a workgroup with nothing for the guarded loop (d) and
splits a workgroup across the loop boundary (e); the edge counts and the cap
of one workgroup are there (f).  The model itself is checked against a
mutation of each loop, so a property it reports is one a wrong kernel would
miss."""
import inspect

import numpy as np
import pytest

import pico_amd
import reduce_variants_cases as C

ESZS = (1, 2, 4, 8, 16)


@pytest.mark.parametrize("U", C.US)
def test_every_vector_is_written_exactly_once(U):
    """(a), for every count and cap of the table and the cap of 2 the other tests use"""
    for nvec in C.counts(U):
        for cap in C.CAPS + (2,):
            blocks = C.blocks_of(nvec, U, cap)
            w = C.written(nvec, U, blocks)
            assert (w[:nvec] == 1).all() and w[nvec] == 0, (U, nvec, cap, blocks)


@pytest.mark.parametrize("U", C.US)
def test_multi_trip_shape_reaches_b_to_e(U):
    t, n = C.tile(U), C.multi(U)
    assert n == 7 * t + 256 * (U - 1) + 100 and n in C.counts(U)
    for cap in (2, 3):
        assert C.blocks_of(n, U, cap) == cap
        assert C.reaches(n, U, cap) == {"b", "c", "d", "e"}, (U, cap)
    # tile 7 of the cap-3 launch: workgroup 1, lanes below 100 in a trip, the others in the guarded loop
    lanes = C.walk(n, U, 3)[1]
    for lane, (trips, guarded, base) in enumerate(lanes):
        took = [x[0] - lane for x in trips]
        if lane < 100:
            assert took == [t, 4 * t, 7 * t] and not guarded and base >= n
        else:
            assert took == [t, 4 * t] and base == 7 * t + lane
            assert guarded == [base + u * 256 for u in range(U - 1)]
    # workgroup 0 takes three trips and leaves past the end, whatever the lane
    assert all(len(trips) == 3 and not guarded and base >= n for trips, guarded, base in C.walk(n, U, 3)[0])
    # one workgroup walks everything; the default cap gives one trip per workgroup at most
    assert C.blocks_of(n, U, 1) == 1 and "b" in C.reaches(n, U, 1)
    assert C.blocks_of(n, U, 0) == 8 and "b" not in C.reaches(n, U, 8)
    # the guarded loop of U = 1 can never write: its partial tile is taken by the loop itself
    if U == 1:
        assert all(not g for nv in C.counts(1) for cap in C.CAPS + (2,)
                   for lanes in C.walk(nv, 1, C.blocks_of(nv, 1, cap)) for _, g, _ in lanes)


@pytest.mark.parametrize("U", C.US)
def test_partial_shape_and_edges(U):
    t = C.tile(U)
    # (c) alone: workgroup 1 of the cap-3 launch ends on 100 vectors that (U >= 2) no lane takes as a trip
    got = C.reaches(C.partial(U), U, 3)
    assert {"b", "c", "d"} <= got and (("e" in got) == (U == 1)), (U, got)
    # ... and, under a cap of 2 or 3, the last vector is the guarded loop's (in the multi-trip shape a trip's)
    for cap in (2, 3):
        last = {nv: [bool(g) for lanes in C.walk(nv, U, cap) for _, g, _ in lanes if nv - 1 in g]
                for nv in (C.partial(U), C.multi(U))}
        assert last == {C.partial(U): [True] if U > 1 else [], C.multi(U): []}, (U, cap, last)
        assert "c" in C.reaches(C.partial(U), U, cap)
    # (f)
    assert set(C.counts(U)) >= {0, 1, t - 1, t, t + 1} and 1 in C.CAPS and 0 in C.CAPS
    assert C.blocks_of(0, U, 3) == 1 and C.blocks_of(1, U, 0) == 1 and C.blocks_of(t + 1, U, 0) == 2
    assert C.blocks_of(t + 1, U, 1) == 1 and C.reaches(t + 1, U, 1) >= ({"b"} if U == 1 else {"c"})
    assert C.blocks_of(1 << 40, U, 0) == C.DEFAULT_CAP == 16384
    # the largest case: U = 8 at about 8 tiles
    assert max(C.counts(U)) * 16 <= 8 * C.tile(8) * 16 == 256 << 10


def test_the_model_tells_the_mutations_apart():
    """the full-tile loop run once only, and the guarded loop stopping one vector early, each break
    (a) on the shapes above -- and the first only where a second trip exists"""
    U, n = 4, C.multi(4)

    def once(nvec, blocks):            # `for` -> `if`
        w = np.zeros(nvec + 1, dtype=np.int64)
        for wg in range(blocks):
            for lane in range(C.KBLOCK):
                base = wg * C.tile(U) + lane
                if base + (U - 1) * C.KBLOCK < nvec:
                    for u in range(U):
                        w[base + u * C.KBLOCK] += 1
                    base += blocks * C.tile(U)
                for u in range(U):
                    if base + u * C.KBLOCK < nvec:
                        w[base + u * C.KBLOCK] += 1
        return w

    assert (once(n, 8)[:n] == 1).all()                  # one trip per workgroup: the mutation does not show
    assert (once(n, 3)[:n] == 0).any()                  # capped: vectors are left out
    w = C.written(n - 1, U, 3)                          # `i < nvec` -> `i + 1 < nvec` is the walk of nvec - 1 ...
    assert w[n - 1] == 0 and (w[:n - 1] == 1).all()     # ... which leaves the last vector out


@pytest.mark.parametrize("esz", ESZS)
def test_element_counts_give_the_vector_counts(esz):
    per = 16 // esz
    for U in C.US:
        for nvec in C.counts(U):
            for phase in C.PHASES:
                n = C.elements(nvec, esz, phase)
                head, nv = C.split(phase * esz, n, esz)
                assert nv == nvec and head == (per - 1 if phase and n else 0), (esz, U, nvec, phase)
                tail = n - head - nvec * per
                assert (1 <= tail < per) if phase and per > 1 else tail == 0
    assert [C.elements(0, 4, 1), C.split(4, C.elements(0, 4, 1), 4)] == [4, (3, 0)]   # float: head 3, tail 1


def test_arena_guards_and_phases():
    a, b = np.arange(37, dtype=np.float32), np.arange(37, dtype=np.float32) + 100
    for phases in ((0, 0, 0), (1, 1, 1), (1, 0, 3)):
        ar = C.Arena(a, b, phases)
        assert ar.init.size % 64 == 0
        edges = sorted((o, o + 37 * 4) for o in ar.off)
        assert edges[0][0] >= C.GUARD_BYTES and ar.init.size - edges[-1][1] >= C.GUARD_BYTES
        assert all(nxt[0] - cur[1] >= 2 * C.GUARD_BYTES for cur, nxt in zip(edges, edges[1:]))
        assert [o % 16 for o in ar.off] == [4 * p for p in phases]
        used = np.zeros(ar.init.size, dtype=bool)
        for lo, hi in edges[:2] if ar.off[2] == edges[2][0] else edges:
            used[lo:hi] = True
        assert (ar.init[~used] == C.GUARD).all()
        assert ar.init[ar.off[0]:ar.off[0] + 148].tobytes() == a.tobytes()
        img = ar.expected(a + b, inplace=True)
        assert img[ar.off[1]:ar.off[1] + 148].tobytes() == (a + b).tobytes()
        assert (img[ar.off[2]:ar.off[2] + 148] == C.GUARD).all()
        assert ar.where(ar.off[2] + 5) == "out[1]" and ar.where(ar.off[1] - 1) == "1 bytes before b"


def test_tuning_reset_is_the_library_default():
    """set_reduce_tuning() with no argument restores the library's defaults (kDefaultUnroll, the
    default cap, kDefaultNT: non-temporal loads of the once-read operand)"""
    p = inspect.signature(pico_amd.set_reduce_tuning).parameters
    assert [p[k].default for k in ("unroll", "maxblocks", "nontemporal")] == [C.DEFAULT_U, 0, 1]
