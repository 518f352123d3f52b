"""Dynamic loss scaling, host side: bine_step_update_host and bine_step_state_init
against tests/step_sim.py (the header's update rule in numpy, one float64
operation per line) on all 96 bytes, the state's constants against
bine_adamw_consts, and every refusal of the new entry points reached through
ctypes.  No GPU: every call below ends before its first HIP call."""
import ctypes
import math

import numpy as np
import pytest

import pico_amd
import step_sim as S
from pico_amd import _lib
from pico_amd._lib import ALGOS, DTYPES, EXT_DTYPES, BineError

ERR_ARG, ERR_UNSUPPORTED = 1, 6
CODE = {**DTYPES, **EXT_DTYPES}
INF, NAN = float("inf"), float("nan")
# the hyper-parameters of DESIGN.md 6.7's measurements and tests
HYPER67 = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def betas(hyper):
    h = dict(S.HYPER, **hyper)
    return h["beta1"], h["beta2"]


def run_case(init, hyper, norms):
    """the library's and the sim's states after every update, compared on all bytes"""
    scale, step = init
    got = pico_amd.step_state_init(scale, step, *betas(hyper))
    want = S.init(scale, step, *betas(hyper))
    assert got.dtype == np.uint8 and got.size == S.BYTES
    assert got.tobytes() == want.tobytes(), "init"
    trace = [S.fields(want)]
    for i, n2 in enumerate(norms):
        pico_amd.step_update_host(got, n2, **hyper)
        want = S.update(want, n2, **hyper)
        assert got.tobytes() == want.tobytes(), (i, n2, S.fields(got), S.fields(want))
        trace.append(S.fields(want))
    return trace


@pytest.mark.parametrize("case", S.cases(), ids=lambda c: c[0])
def test_update_host_is_the_sim_on_every_byte(case):
    name, init, hyper, norms = case
    assert len(norms) >= 200
    kinds = {"inf": any(x == INF for x in norms), "nan": any(math.isnan(x) for x in norms),
             "zero": any(x == 0.0 for x in norms), "finite": any(0.0 < x < INF for x in norms)}
    trace = run_case(init, hyper, norms)
    last = trace[-1]
    bad = sum(1 for x in norms if not x <= S.DBL_MAX)
    assert last["skipped"] == bad and last["step"] == init[1] + len(norms) - bad
    if name in ("defaults, max_norm = inf", "clipping", "beta1 = 0", "resumed at step 1000"):
        assert all(kinds.values()), kinds
    # a skipped update: step, pw1, pw2 and c[] untouched, skip = 1, gm = 0
    for n2, a, b in zip(norms, trace, trace[1:]):
        if not n2 <= S.DBL_MAX:
            assert b["skip"] == 1.0 and b["gm"] == 0.0 and b["good"] == 0.0
            assert (b["step"], b["pw1"], b["pw2"]) == (a["step"], a["pw1"], a["pw2"])
            assert b["consts"].tobytes() == a["consts"].tobytes()
            assert b["scale"] <= a["scale"]
        else:
            assert b["skip"] == 0.0 and b["step"] == a["step"] + 1 and b["gm"] > 0.0


def test_growth_exactly_at_the_interval():
    """growth_interval = 5: four good updates and an overflow leave the scale
    halved, never doubled; the fifth good update in a row doubles it"""
    _, init, hyper, norms = next(c for c in S.cases() if c[0] == "growth at the interval")
    t = run_case(init, hyper, norms[:16])
    scales = [x["scale"] for x in t]
    assert scales[:5] == [8.0] * 5 and [x["good"] for x in t[:5]] == [0.0, 1.0, 2.0, 3.0, 4.0]   # one before: no growth
    assert scales[5] == 4.0 and t[5]["good"] == 0.0                                              # the overflow
    assert scales[6:10] == [4.0] * 4 and scales[10] == 8.0 and t[10]["good"] == 0.0              # exactly at 5
    assert scales[11] == 4.0                                                                     # the NaN
    assert scales[12:16] == [4.0] * 4 and scales[16] == 2.0


def test_scale_clamps():
    _, init, hyper, norms = next(c for c in S.cases() if c[0] == "min_scale")
    t = run_case(init, hyper, norms)
    assert [x["scale"] for x in t[:5]] == [4.0, 2.0, 1.0, 0.75, 0.75] and t[-1]["scale"] == 0.75
    _, init, hyper, norms = next(c for c in S.cases() if c[0] == "max_scale")
    t = run_case(init, hyper, norms)
    # 2^22 * 3 = 1.5 * 2^23 < 2^24, * 3 overshoots: clamped; after the overflow half of it, then clamped again
    assert [x["scale"] for x in t[:4]] == [2.0 ** 22, 3 * 2.0 ** 22, 2.0 ** 24, 2.0 ** 24]
    assert t[101]["scale"] == 2.0 ** 23 and t[102]["scale"] == 2.0 ** 24


def test_gm_is_the_clip_rule_on_the_unscaled_norm():
    """max_norm = inf: gm = 1 / scale; max_norm finite: cc from sqrt(n2) / scale,
    bine_clip_segments' expression"""
    st = pico_amd.step_state_init(1024.0, 0, 0.9, 0.999)
    pico_amd.step_update_host(st, 1e30)
    assert pico_amd.step_state_read(st)["gm"] == 1.0 / 1024.0
    st = pico_amd.step_state_init(1024.0, 0, 0.9, 0.999)
    pico_amd.step_update_host(st, 9.0 * 1024.0 ** 2, max_norm=1.5, clip_eps=0.0)      # the true norm is 3
    f = pico_amd.step_state_read(st)
    assert f["gm"] == 0.5 / 1024.0 and f["skip"] == 0.0 and f["step"] == 1.0 and f["good"] == 1.0
    assert sorted(f) == sorted(S.FIELDS + ("consts",))
    st = pico_amd.step_state_init(1.0, 0, 0.9, 0.999)
    pico_amd.step_update_host(st, 0.0, max_norm=0.0, clip_eps=0.0)                    # 0 / 0: NaN r, cc = 1
    assert pico_amd.step_state_read(st)["gm"] == 1.0


@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.0, 0.5), (1.0 / 3.0, 0.999999)])
def test_init_at_step_t_is_t_updates_products(b1, b2):
    hyper = dict(beta1=b1, beta2=b2, growth_interval=10 ** 9)
    run = pico_amd.step_state_init(2.0, 0, b1, b2)
    for t in range(0, 1201):
        if t in (0, 1, 2, 7, 100, 999, 1200):
            got = pico_amd.step_state_init(2.0, t, b1, b2)
            assert got.tobytes() == S.init(2.0, t, b1, b2).tobytes(), t
            a, b = S.fields(got), S.fields(run)
            assert (a["step"], a["pw1"], a["pw2"]) == (b["step"], b["pw1"], b["pw2"]) and a["step"] == t, t
        pico_amd.step_update_host(run, 1.0, **hyper)


def test_init_far_past_the_products_underflow():
    """the loop's early exit changes nothing: 0.75 times a subnormal of two units
    rounds back to it, a fixed point that is not zero; 0.25's product reaches 0"""
    big = S.fields(pico_amd.step_state_init(2.0, 10 ** 12, 0.75, 0.25))
    at3000, at3001 = S.fields(S.init(2.0, 3000, 0.75, 0.25)), S.fields(S.init(2.0, 3001, 0.75, 0.25))
    assert at3000["pw1"] == at3001["pw1"] == 1e-323 and at3000["pw2"] == 0.0
    assert big["step"] == 1e12 and big["pw1"] == at3000["pw1"] and big["pw2"] == 0.0


def ulps(a, b):
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


def test_consts_against_adamw_consts_for_2000_steps():
    """steps 1..2,000 at DESIGN.md 6.7's hyper-parameters: dk, b1, 1 - b1, b2,
    1 - b2 and eps equal bine_adamw_consts', rbc2 and ss within one float32 ulp
    and equal at step 1.  The running products' relative error after t steps is
    at most t * 2^-53, 1 - pw amplifies it by at most 1 / (1 - beta) = 1,000, and
    2,000 * 1,000 * 2^-53 = 2.2e-10 is far below half a float32 ulp (3e-8), so
    only a value that sits within that of a rounding boundary can differ, by one
    ulp -- as pow's own last-place error allows on the other side."""
    st = pico_amd.step_state_init(65536.0, 0, HYPER67["beta1"], HYPER67["beta2"])
    worst = 0
    for t in range(1, 2001):
        pico_amd.step_update_host(st, 1.0, growth_interval=10 ** 9, **HYPER67)
        got = pico_amd.step_state_read(st)
        want = pico_amd.adamw_consts(step=t, **HYPER67)
        assert got["step"] == t
        for j in (0, 1, 2, 3, 4, 6):
            assert got["consts"][j].tobytes() == want[j].tobytes(), (t, j)
        for j in (5, 7):
            u = ulps(got["consts"][j], want[j])
            worst = max(worst, u)
            assert u <= (0 if t == 1 else 1), (t, j, got["consts"][j], want[j])
    print(f"c[5], c[7] over 2,000 steps: at most {worst} ulp from bine_adamw_consts")


# ---- refusals ------------------------------------------------------------------------------

def refused(fn, *a, **k):
    with pytest.raises(BineError) as ei:
        fn(*a, **k)
    return ei.value.status


def test_state_init_refusals():
    for bad in (0.0, -1.0, INF, NAN):
        assert refused(pico_amd.step_state_init, scale=bad) == ERR_ARG
    assert refused(pico_amd.step_state_init, step=-1) == ERR_ARG
    for bad in (-0.1, 1.0, NAN, INF):
        assert refused(pico_amd.step_state_init, beta1=bad) == ERR_ARG
        assert refused(pico_amd.step_state_init, beta2=bad) == ERR_ARG
    L = pico_amd.lib()
    buf = np.zeros(14, dtype=np.float64)
    assert L.bine_step_state_init(None, 1.0, 0, 0.9, 0.999) == ERR_ARG
    assert L.bine_step_state_init(buf.ctypes.data + 4, 1.0, 0, 0.9, 0.999) == ERR_ARG
    assert not buf.any()
    assert L.bine_step_state_init(buf.ctypes.data + 8, 1.0, 0, 0.0, 0.0) == 0 and buf[0] == 0 and buf[13] == 0


BAD_HYPER = [dict(lr=-1e-3), dict(lr=NAN), dict(eps=-1e-8), dict(eps=NAN), dict(weight_decay=-0.01),
             dict(weight_decay=NAN), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=NAN), dict(beta2=1.0),
             dict(beta2=INF), dict(beta2=NAN), dict(max_norm=-1.0), dict(max_norm=NAN), dict(clip_eps=-1e-6),
             dict(clip_eps=NAN), dict(growth_factor=0.999), dict(growth_factor=INF), dict(growth_factor=NAN),
             dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(backoff_factor=1.0001),
             dict(backoff_factor=NAN), dict(growth_interval=0), dict(growth_interval=-3), dict(min_scale=0.0),
             dict(min_scale=-1.0), dict(min_scale=NAN), dict(min_scale=2.0, max_scale=1.0), dict(max_scale=INF),
             dict(max_scale=NAN)]
GOOD_HYPER = [dict(lr=0.0, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0, max_norm=0.0, clip_eps=0.0),
              dict(growth_factor=1.0, backoff_factor=1.0, growth_interval=1, min_scale=3.0, max_scale=3.0),
              dict(max_norm=INF, lr=INF)]


def hyper_struct(**k):
    h = dict(S.HYPER, **k)
    return _lib.StepHyper(*[h[f] for f, _ in _lib.StepHyper._fields_])


def test_update_refusals_host_and_device_entry():
    """bine_step_update refuses before any HIP call, so the device entry point's
    checks run here with made-up aligned addresses"""
    L = pico_amd.lib()
    fresh = pico_amd.step_state_init()
    for bad in BAD_HYPER:
        st = fresh.copy()
        assert refused(pico_amd.step_update_host, st, 1.0, **bad) == ERR_ARG, bad
        assert st.tobytes() == fresh.tobytes(), bad
        assert L.bine_step_update(0x10000, 0x20000, ctypes.byref(hyper_struct(**bad)), None) == ERR_ARG, bad
    for good in GOOD_HYPER:
        pico_amd.step_update_host(fresh.copy(), 1.0, **good)
    h = ctypes.byref(hyper_struct())
    buf = np.zeros(14, dtype=np.float64)
    assert L.bine_step_update_host(None, 1.0, h) == ERR_ARG
    assert L.bine_step_update_host(buf.ctypes.data + 4, 1.0, h) == ERR_ARG
    assert L.bine_step_update_host(buf.ctypes.data, 1.0, None) == ERR_ARG
    for state, norm2 in ((None, 0x20000), (0x10004, 0x20000), (0x10000, None), (0x10000, 0x20004)):
        assert L.bine_step_update(state, norm2, h, None) == ERR_ARG, (state, norm2)
    assert L.bine_step_update(0x10000, 0x20000, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        pico_amd.step_update_host(np.zeros(95, dtype=np.uint8), 1.0)


def dyn(n, p, m, v, g, pout, counts, state, gd="float", od="float"):
    arr = lambda a: None if a is None else (ctypes.c_void_p * max(len(a), 1))(*a)  # noqa: E731
    c = None if counts is None else (ctypes.c_size_t * max(len(counts), 1))(*counts)
    return pico_amd.lib().bine_adamw_segments_dyn(n, arr(p), arr(m), arr(v), arr(g), arr(pout), c, CODE[gd],
                                                  CODE[od], state, None)


def test_adamw_segments_dyn_refusals():
    A, ST = [0x1000], 0x9000
    assert dyn(1, A, A, A, A, A, [4], None) == ERR_ARG                     # state NULL
    assert dyn(1, A, A, A, A, A, [4], ST + 4) == ERR_ARG                   # not 8-byte aligned
    assert dyn(0, None, None, None, None, None, None, None) == ERR_ARG     # also with nothing to do
    # adamw_args' list checks, a valid state behind them
    assert dyn(-1, A, A, A, A, A, [4], ST) == ERR_ARG
    assert dyn(_lib.MULTI_MAX + 1, A, A, A, A, A, [4], ST) == ERR_ARG
    for which in range(4):
        q = [A, A, A, A]
        q[which] = None
        assert dyn(1, *q, A, [4], ST) == ERR_ARG
        q[which] = [None]
        assert dyn(1, *q, A, [4], ST) == ERR_ARG                           # NULL with a non-zero count
        q[which] = [0x1002]
        assert dyn(1, *q, A, [4], ST) == ERR_ARG                           # not a float's alignment
    assert dyn(1, A, A, A, A, A, None, ST) == ERR_ARG
    assert dyn(1, A, A, A, A, [0x1001], [4], ST, od="bfloat16") == ERR_ARG
    assert dyn(1, A, A, A, A, A, [4], ST, gd="double") == ERR_ARG
    assert dyn(1, A, A, A, A, None, [4], ST, od="int32") == ERR_ARG
    with pytest.raises(ValueError):
        pico_amd.adamw_segments_dyn([1], [1, 2], [1], [1], 0x9000, counts=[4])


def test_adamw_multi_dyn_refusals():
    """the list checks and the state first, then the allgather's, then the communicator"""
    L = pico_amd.lib()
    A = (ctypes.c_void_p * 1)(0x1000)
    c = (ctypes.c_size_t * 1)(4)
    ring = ALGOS["allgather"]["ring"]
    call = lambda comm, algo, state, counts=c, g=A: L.bine_adamw_multi_dyn(  # noqa: E731
        comm, algo, 1, A, A, A, A, g, counts, CODE["float"], CODE["bfloat16"], state, None)
    assert call(None, ring, None) == ERR_ARG
    assert call(None, ring, 0x9004) == ERR_ARG
    assert call(None, ring, 0x9000, g=None) == ERR_ARG
    assert call(None, 9999, 0x9000) == ERR_UNSUPPORTED                     # the allgather's algorithm range
    assert call(None, ring, 0x9000, counts=(ctypes.c_size_t * 1)(2 ** 31)) == ERR_ARG
    assert call(None, ring, 0x9000) == ERR_ARG                             # comm == NULL, last
    st = (ctypes.c_int * 2)(7, 7)
    lb = lambda states: L.bine_loopback_run_adamw_multi_dyn(  # noqa: E731
        None, 2, ring, 0, None, None, None, None, None, None, CODE["float"], CODE["float"], states, st)
    assert lb(None) == ERR_ARG and list(st) == [ERR_ARG, ERR_ARG]
    assert lb((ctypes.c_void_p * 2)(0x9000, 0x9004)) == ERR_ARG
