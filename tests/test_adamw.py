"""Fused AdamW step, host side: bine_adamw_consts against numpy's
float64-then-float32 statement, bine_plan_adamw against a Python restatement of
the tile rule, the launch cut and the body flag, and every refusal of
bine_adamw_segments / bine_plan_adamw / bine_adamw_multi and its loopback driver
reached through ctypes.  No GPU: every call below ends before its first HIP
call."""
import ctypes
import math

import numpy as np
import pytest

import pico_amd
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, BineError

ERR_ARG, ERR_UNSUPPORTED = 1, 6
S = _lib.ADAMW_SEGS_PER_LAUNCH
CODE = {**DTYPES, **EXT_DTYPES}
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TILE_VECS = 2048          # kBlock * kScaleU 16-B vectors of p: 8,192 elements
TILE = TILE_VECS * 4
COUNTS = [0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 21]
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


# ---- bine_adamw_consts ---------------------------------------------------------------------

def np_consts(lr, beta1, beta2, eps, weight_decay, step):
    """float64 throughout, one rounding to float32 each"""
    lr, b1, b2, eps, wd = (np.float64(x) for x in (lr, beta1, beta2, eps, weight_decay))
    one = np.float64(1.0)
    return np.array([one - lr * wd, b1, one - b1, b2, one - b2, one / np.sqrt(one - b2 ** np.float64(step)), eps,
                     lr / (one - b1 ** np.float64(step))], dtype=np.float64).astype(np.float32)


def ulps(a, b):
    """distance of two positive finite float32 in units of the last place"""
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


CONST_CASES = [HYPER, dict(lr=3e-4, beta1=0.95, beta2=0.98, eps=1e-6, weight_decay=0.0),
               dict(lr=0.1, beta1=0.0, beta2=0.5, eps=0.0, weight_decay=0.3),
               dict(lr=1.0 / 3.0, beta1=1.0 / 3.0, beta2=2.0 / 3.0, eps=1e-30, weight_decay=1e-7)]


@pytest.mark.parametrize("hyper", CONST_CASES)
def test_consts_are_float64_then_float32(hyper):
    for step in (1, 2, 10, 1000, 10 ** 6):
        got, want = pico_amd.adamw_consts(step=step, **hyper), np_consts(step=step, **hyper)
        assert got.dtype == np.float32 and got.shape == (8,)
        for j in (0, 1, 2, 3, 4, 6):           # dk, b1, 1 - b1, b2, 1 - b2, eps: exactly
            assert got[j].tobytes() == want[j].tobytes(), (step, j, got[j], want[j])
        for j in (5, 7):                       # rbc2, ss: pow is not required to be correctly rounded
            assert np.isfinite(got[j]) and got[j] > 0
            print(f"step {step} const {j}: {got[j]!r} against {want[j]!r}, {ulps(got[j], want[j])} ulp")
            assert ulps(got[j], want[j]) <= (0 if step == 1 else 1), (step, j, got[j], want[j])


def test_consts_refusals():
    L = pico_amd.lib()
    out = (ctypes.c_float * 8)()
    ok = dict(HYPER, step=1)

    def call(out=out, **kw):
        a = dict(ok, **kw)
        return L.bine_adamw_consts(a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"], a["step"], out)

    assert call() == 0
    nan = float("nan")
    for name in ("lr", "eps", "weight_decay"):
        assert call(**{name: -1e-300}) == ERR_ARG and call(**{name: nan}) == ERR_ARG
        assert call(**{name: 0.0}) == 0
    for name in ("beta1", "beta2"):
        for bad in (-1e-300, 1.0, 1.5, nan, float("inf")):
            assert call(**{name: bad}) == ERR_ARG, (name, bad)
        assert call(**{name: 0.0}) == 0 and call(**{name: math.nextafter(1.0, 0.0)}) == 0
    assert call(step=0) == ERR_ARG and call(step=-5) == ERR_ARG
    assert call(out=None) == ERR_ARG
    with pytest.raises(BineError):
        pico_amd.adamw_consts(step=0, **HYPER)


# ---- bine_plan_adamw -----------------------------------------------------------------------

def tiles_of(addr, count):
    """the tile rule over p as float32: the elements before p's first 16-B
    boundary and after its last full vector go with the first workgroup; one
    workgroup per 2,048 vectors in between, at least one per non-empty tensor"""
    if count == 0:
        return 0
    head = min(((16 - addr % 16) % 16) // 4, count)
    return max(1, -(-((count - head) // 4) // TILE_VECS))


def body_of(p, m, v, g, pout, gsz, osz):
    """0 (vector) when every operand stands on a boundary of its own 4-element
    vector where p stands on a 16-B one, else 1 (element)"""
    h = ((16 - p % 16) % 16) // 4
    vec = (m + 4 * h) % 16 == 0 and (v + 4 * h) % 16 == 0 and (g + gsz * h) % (4 * gsz) == 0
    if pout is not None:
        vec = vec and (pout + osz * h) % (4 * osz) == 0
    return 0 if vec else 1


def want_plan(p, m, v, g, pout, counts, gsz, osz):
    """records in launch order: a launch per 64 non-empty segments"""
    recs, slot, launch, wg = [], 0, 0, 0
    for k, c in enumerate(counts):
        if c == 0:
            continue
        if slot == S:
            slot, launch, wg = 0, launch + 1, 0
        t = tiles_of(p[k], c)
        recs.append((launch, k, wg, t, body_of(p[k], m[k], v[k], g[k], None if pout is None else pout[k], gsz, osz)))
        slot, wg = slot + 1, wg + t
    return recs


def addrs(base, n, esz, phases):
    return [base + 0x100000 * k + esz * phases[k] for k in range(n)]


@pytest.mark.parametrize("gdtype", sorted(ESZ))
@pytest.mark.parametrize("odtype", sorted(ESZ))
def test_plan_adamw_tiles_and_body(gdtype, odtype):
    gsz, osz, n = ESZ[gdtype], ESZ[odtype], len(COUNTS)
    for phase in range(4):
        ph = [phase] * n
        p = addrs(0x10000000, n, 4, ph)
        cong = dict(m=addrs(0x20000000, n, 4, ph), v=addrs(0x30000000, n, 4, ph), g=addrs(0x40000000, n, gsz, ph),
                    pout=addrs(0x50000000, n, osz, ph))
        off = [(phase + 1) % 4] * n
        cases = [("congruent", cong, 0), ("m off", dict(cong, m=addrs(0x20000000, n, 4, off)), 1),
                 ("v off", dict(cong, v=addrs(0x30000000, n, 4, off)), 1),
                 ("g off", dict(cong, g=addrs(0x40000000, n, gsz, off)), 1),
                 ("pout off", dict(cong, pout=addrs(0x50000000, n, osz, off)), 1),
                 ("pout absent", dict(cong, pout=None), 0),
                 ("pout absent, g off", dict(cong, pout=None, g=addrs(0x40000000, n, gsz, off)), 1)]
        for name, a, body in cases:
            got = pico_amd.plan_adamw(p, a["m"], a["v"], a["g"], a["pout"], COUNTS, gdtype, odtype)
            want = want_plan(p, a["m"], a["v"], a["g"], a["pout"], COUNTS, gsz, osz)
            assert got == want, (name, phase)
            assert [r[4] for r in got] == [body] * (n - 1), (name, phase)
            assert [r[3] for r in got] == [tiles_of(x, c) for x, c in zip(p, COUNTS) if c]
    # one element past a tile is a tail element; one vector past it is a second tile, unless p's
    # phase splits that vector into a head and a tail
    one = lambda a, c: pico_amd.plan_adamw([a], [a], [a], [a], None, [c], "float")[0][3]  # noqa: E731
    assert one(0x1000, TILE + 1) == 1 and one(0x1000, TILE + 4) == 2 and one(0x1004, TILE + 4) == 1
    # 16-bit g against p's phase: g's 4-element vector is 8 B, so p at phase 1 wants g at 6 mod 8
    assert pico_amd.plan_adamw([0x1004], [0x2004], [0x3004], [0x4002], None, [64], "bfloat16")[0][4] == 0
    assert pico_amd.plan_adamw([0x1004], [0x2004], [0x3004], [0x400A], None, [64], "bfloat16")[0][4] == 0
    assert pico_amd.plan_adamw([0x1004], [0x2004], [0x3004], [0x4004], None, [64], "bfloat16")[0][4] == 1


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 37])
def test_plan_adamw_list_lengths(n):
    """launch boundaries at 64 non-empty segments; empties (some NULL) in between"""
    rng = np.random.default_rng(n)
    p, m, v, g, o, counts = [], [], [], [], [], []
    for k in range(n):
        ph = int(rng.integers(0, 4))
        mph = ph if k % 7 else (ph + 1) % 4
        p.append(0x10000000 + 0x10000 * k + 4 * ph)
        m.append(0x20000000 + 0x10000 * k + 4 * mph)
        v.append(0x30000000 + 0x10000 * k + 4 * ph)
        g.append(0x40000000 + 0x10000 * k + 2 * ph)
        o.append(0x50000000 + 0x10000 * k + 2 * ph)
        counts.append(int(rng.choice([1, 3, 4, 5, 100, 1025, TILE + 9])))
        if k % 5 == 0:                                       # an empty, NULL every other time
            null = k % 10 == 0
            for lst in (p, m, v, g, o):
                lst.append(0 if null else 0x60000000)
            counts.append(0)
    got = pico_amd.plan_adamw(p, m, v, g, o, counts, "float16", "bfloat16")
    want = want_plan(p, m, v, g, o, counts, 2, 2)
    assert got == want and len(got) == n
    assert [r[0] for r in got] == [j // S for j in range(n)]
    for j, r in enumerate(got):
        if j % S == 0:
            assert r[2] == 0                                 # tile0 rebased at every launch
    if n:
        assert {r[4] for r in got} == ({0, 1} if n >= 8 else {r[4] for r in want})
    # cap below the count: the count is returned, nothing past cap is written
    L = pico_amd.lib()
    arr = lambda a: (ctypes.c_uint64 * max(len(a), 1))(*a)  # noqa: E731
    out = (ctypes.c_uint64 * 10)(*([0xDEAD] * 10))
    r = L.bine_plan_adamw(len(counts), arr(p), arr(m), arr(v), arr(g), arr(o),
                          (ctypes.c_size_t * max(len(counts), 1))(*counts), CODE["float16"], CODE["bfloat16"], out, 1)
    assert r == n and list(out[5:]) == [0xDEAD] * 5
    if n:
        assert tuple(out[:5]) == want[0]


# ---- refusals, in the header's order -------------------------------------------------------

def test_adamw_refusals():
    L = pico_amd.lib()
    big = _lib.MULTI_MAX + 1
    f, h, b = CODE["float"], CODE["float16"], CODE["bfloat16"]
    pv = (ctypes.c_void_p * big)(*([0x1000] * big))
    pu = (ctypes.c_uint64 * big)(*([0x1000] * big))
    cnt = (ctypes.c_size_t * big)(*([4] * big))
    null, nullu = (ctypes.c_void_p * 1)(None), (ctypes.c_uint64 * 1)(0)
    zero = (ctypes.c_size_t * 1)(0)
    NAMES = ("p", "m", "v", "g", "pout")

    def seg(n=1, counts=cnt, gdtype=f, odtype=f, gcoef=None, grad_mul=1.0, step=1, **kw):
        a = {k: kw.pop(k, pv) for k in NAMES}
        hy = dict(HYPER, **kw)
        return L.bine_adamw_segments(n, a["p"], a["m"], a["v"], a["g"], a["pout"], counts, gdtype, odtype, hy["lr"],
                                     hy["beta1"], hy["beta2"], hy["eps"], hy["weight_decay"], step, gcoef, grad_mul,
                                     None)

    def plan(n=1, counts=cnt, gdtype=f, odtype=f, **kw):
        u = {k: kw.pop(k, pv) for k in NAMES}
        u = {k: None if x is None else nullu if x is null else pu if x is pv else x for k, x in u.items()}
        assert not kw
        return -L.bine_plan_adamw(n, u["p"], u["m"], u["v"], u["g"], u["pout"], counts, gdtype, odtype, None, 0)

    # the element types: float, float16, bfloat16 -- before a bad n is looked at
    for d in sorted(CODE.values()) + [-1, 17, 31, 34]:
        if d in (f, h, b):
            assert L.bine_plan_adamw(1, pu, pu, pu, pu, pu, cnt, d, f, None, 0) == 1
            assert L.bine_plan_adamw(1, pu, pu, pu, pu, None, cnt, f, d, None, 0) == 1
            continue
        for call in (seg, plan):
            assert call(gdtype=d) == ERR_ARG and call(odtype=d) == ERR_ARG
            assert call(n=-1, gdtype=d) == ERR_ARG and call(odtype=d, pout=None) == ERR_ARG
    for call in (seg, plan):
        assert call(n=-1) == ERR_ARG and call(n=big) == ERR_ARG
        assert call(counts=None) == ERR_ARG
        for name in ("p", "m", "v", "g"):
            assert call(**{name: None}) == ERR_ARG, name              # a NULL array with n > 0
        for name in NAMES:
            assert call(**{name: null}) == ERR_ARG, name              # a NULL buffer with a non-zero count
    # ... which is fine for an empty segment, and pout may be NULL as a whole
    assert plan(p=null, m=null, v=null, g=null, pout=null, counts=zero) == 0
    assert plan(pout=None) == -1 and plan(n=0, p=None, m=None, v=None, g=None, pout=None, counts=None) == 0
    # a buffer not aligned to its element size
    for name in NAMES:
        for t, esz in ESZ.items():
            if name in ("p", "m", "v") and t != "float":
                continue
            for off in range(1, 8):
                kw = {name: (ctypes.c_void_p * 1)(0x1000 + off), "gdtype": CODE[t] if name == "g" else f,
                      "odtype": CODE[t] if name == "pout" else f}
                want = ERR_ARG if off % esz else 0
                kwu = dict(kw, **{name: (ctypes.c_uint64 * 1)(0x1000 + off)})
                assert (plan(**kwu) == ERR_ARG) == bool(want), (name, t, off)
                if want:
                    assert seg(**kw) == ERR_ARG, (name, t, off)
    # gcoef not 8-byte aligned; grad_mul NaN, infinite or negative
    assert seg(gcoef=0x2004) == ERR_ARG
    for bad in (float("nan"), float("inf"), -1.0, -1e-300):
        assert seg(grad_mul=bad) == ERR_ARG, bad
    # the refusals of bine_adamw_consts
    nan = float("nan")
    for kw in (dict(lr=-1.0), dict(lr=nan), dict(eps=-1.0), dict(eps=nan), dict(weight_decay=-1.0),
               dict(weight_decay=nan), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0),
               dict(beta2=-0.1), dict(beta2=nan), dict(step=0), dict(step=-1)):
        assert seg(**kw) == ERR_ARG, kw

    # bine_adamw_multi and its loopback driver, no communicator: the same refusals, then the
    # allgather's (a count above INT_MAX, the algorithm id), then comm == NULL
    ag = ALGOS["allgather"]["ring"]

    def multi(algo=ag, n=1, counts=cnt, gdtype=f, odtype=f, gcoef=None, grad_mul=1.0, step=1, **kw):
        a = {k: kw.pop(k, pv) for k in ("params", "p", "m", "v", "g")}
        hy = dict(HYPER, **kw)
        return L.bine_adamw_multi(None, algo, n, a["params"], a["p"], a["m"], a["v"], a["g"], counts, gdtype, odtype,
                                  hy["lr"], hy["beta1"], hy["beta2"], hy["eps"], hy["weight_decay"], step, gcoef,
                                  grad_mul, None)

    def loop(algo=ag, n=1, counts=cnt, gdtype=f, odtype=f, gcoef=None, grad_mul=1.0, step=1, **kw):
        a = {k: kw.pop(k, pv) for k in ("params", "p", "m", "v", "g")}
        hy = dict(HYPER, **kw)
        st = (ctypes.c_int * 2)(-7, -7)
        hs = (ctypes.c_void_p * 2)(None, None)
        gc = None if gcoef is None else (ctypes.c_void_p * 2)(gcoef, gcoef)
        rc = L.bine_loopback_run_adamw_multi(hs, 2, algo, n, a["params"], a["p"], a["m"], a["v"], a["g"], counts,
                                             gdtype, odtype, hy["lr"], hy["beta1"], hy["beta2"], hy["eps"],
                                             hy["weight_decay"], step, gc, grad_mul, st)
        assert list(st) == [rc, rc]
        return rc

    huge = (ctypes.c_size_t * 1)(2 ** 31)
    for call in (multi, loop):
        assert call(gdtype=CODE["double"], algo=-1) == ERR_ARG
        assert call(n=-1, algo=-1) == ERR_ARG
        for name in ("p", "m", "v", "g", "params"):
            assert call(**{name: None}, algo=-1) == ERR_ARG, name
        assert call(params=null, algo=-1) == ERR_ARG and call(g=null, algo=-1) == ERR_ARG
        assert call(params=(ctypes.c_void_p * 2)(0x1002, 0x1002), algo=-1) == ERR_ARG     # float params at 2 mod 4
        assert call(gcoef=0x2004, algo=-1) == ERR_ARG
        assert call(grad_mul=nan, algo=-1) == ERR_ARG
        assert call(step=0, algo=-1) == ERR_ARG and call(beta2=1.0, algo=-1) == ERR_ARG
        assert call(counts=huge, algo=-1) == ERR_ARG
        assert call(algo=-1) == ERR_UNSUPPORTED and call(algo=10 ** 6) == ERR_UNSUPPORTED
    assert multi() == ERR_ARG                                         # comm == NULL, checked last
