"""Dynamic loss scaling on the GPU: bine_step_update (k_step_update) against
tests/step_sim.py on every byte, bine_adamw_segments_dyn (k_adamw_segs' DYN
form) against adamw_sim with the state's constants and against the plain call
at step 1, a skipped step that stores nothing, and the whole float16 chain over
loopback ranks -- reduce-scatter, norm, state update, AdamW plus allgather --
with planted and natural overflows.  (Real processes and graph mode:
tools/step_check.py, tests/test_gpu_step_rccl.py.)"""
import numpy as np
import pytest

import adamw_sim as A
import h16_util as H
import optim_ref as R
import step_sim as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
import test_gpu_adamw as TA  # noqa: E402  (Bucket, Step, Ranks, the layouts)
import test_gpu_norm as TN  # noqa: E402  (Guarded)
import test_gpu_train_step as TS  # noqa: E402  (load, within_bounds)

TILE = TA.TILE
TYPES = TA.TYPES
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class DevState:
    """a state block in device memory, 16 guard bytes on either side"""

    def __init__(self, host_state):
        self.g = TN.Guarded(S.BYTES // 8, fill=np.ascontiguousarray(host_state).view(np.uint64))

    def ptr(self):
        return self.g.ptr()

    def read(self):
        return self.g.read().view(np.uint8)


# ---- bine_step_update ------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.cases(), ids=lambda c: c[0])
def test_step_update_on_the_device_is_the_sim(dev, case):
    """the CPU test's sequences with norm2 in device memory: after every update
    the state's 96 bytes are copied aside on the same stream, one read at the end"""
    _, (scale, step), hyper, norms = case
    h = dict(S.HYPER, **hyper)
    st = DevState(pico_amd.step_state_init(scale, step, h["beta1"], h["beta2"]))
    n2 = TN.Guarded(len(norms), fill=np.array(norms, dtype=np.float64).view(np.uint64))
    log = torch.zeros(len(norms), S.BYTES, dtype=torch.uint8, device="cuda:0")
    view = st.g.t[2:2 + S.BYTES // 8].view(torch.uint8)
    for i in range(len(norms)):
        pico_amd.step_update(st.ptr(), n2.ptr() + 8 * i, **hyper)
        log[i].copy_(view)
    torch.cuda.synchronize()
    got = log.cpu().numpy()
    want = S.init(scale, step, h["beta1"], h["beta2"])
    for i, x in enumerate(norms):
        want = S.update(want, x, **hyper)
        assert got[i].tobytes() == want.tobytes(), (i, x, S.fields(got[i]), S.fields(want))
    assert st.read().tobytes() == want.tobytes()                       # and the guards
    assert n2.read().tobytes() == np.array(norms, dtype=np.float64).tobytes()
    assert pico_amd.step_state_read(view)["step"] == S.fields(want)["step"]


# ---- bine_adamw_segments_dyn -----------------------------------------------------------------

def host_state(scale, step, n2, **hyper):
    h = dict(S.HYPER, **hyper)
    st = pico_amd.step_state_init(scale, step, h["beta1"], h["beta2"])
    pico_amd.step_update_host(st, n2, **hyper)
    assert st.tobytes() == S.update(S.init(scale, step, h["beta1"], h["beta2"]), n2, **hyper).tobytes()
    return st


# a first step without clipping (gm = 2^-10 exactly) and a late, clipped one (gm and all of c[] inexact)
STATES = [dict(scale=1024.0, step=0, n2=1e9),
          dict(scale=4096.0, step=999, n2=3e12, max_norm=1.0, lr=3e-2, beta1=0.8, beta2=0.95, eps=1e-6,
               weight_decay=0.0)]


def run_dyn(s, state):
    pico_amd.adamw_segments_dyn(s.p.ptrs(), s.m.ptrs(), s.v.ptrs(), s.g.ptrs(), state.ptr(),
                                pout=None if s.o is None else s.o.ptrs(), gdtype=s.gdtype,
                                odtype=s.odtype or "float", counts=s.counts)
    torch.cuda.synchronize()


def sim_dyn(data, gdtype, odtype, f):
    out = []
    for p, m, v, g in data:
        p2, m1, v1 = A.step(p, m, v, g, gdtype, f["consts"], np.float32(np.float64(f["gm"])))
        r = [p2, m1, v1] + ([A.narrow(p2, odtype)] if odtype is not None else [])
        out.append(tuple(x.view(np.uint8) for x in r))
    return out


@pytest.mark.parametrize("odtype", TA.OUT_TYPES, ids=lambda t: t or "absent")
@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_segments_dyn_is_the_sim_on_both_bodies(dev, gdtype, odtype):
    """skip = 0: p', m', v' and pout bit for bit adamw_sim's with consts = the
    state's c[] and gm = float32(d[6]), on test_gpu_adamw's nine counts at every
    phase (vector body) and with one operand off p's phase (element body): head,
    tail, partial and full tiles; guard bytes, g and the state untouched"""
    counts, aph, nulls = TA.aligned_layout()
    _, mph, _ = TA.mixed_layout(3)
    data = TA.tensors(counts, 11, gdtype)
    for kw in STATES:
        hs = host_state(**kw)
        f = S.fields(hs)
        assert f["skip"] == 0.0 and f["step"] == kw["step"] + 1
        want = sim_dyn(data, gdtype, odtype, f)
        for name, phases in (("vector", aph), ("element", mph)):
            s = TA.Step(counts, phases, nulls, data, gdtype, odtype)
            st = DevState(hs)
            run_dyn(s, st)
            TA.same_bits(s.results(), want, (name, kw["step"]))
            assert st.read().tobytes() == hs.tobytes()
    # the state matters: the two give other bits
    assert sim_dyn(data, gdtype, odtype, S.fields(host_state(**STATES[0])))[8][0].tobytes() != want[8][0].tobytes()


@pytest.mark.parametrize("gdtype", ["float", "float16"])
def test_adamw_segments_dyn_at_step_1_is_the_plain_call(dev, gdtype):
    """the first step with clipping: adamw_segments(gcoef -> cc on the device,
    grad_mul = inv, step = 1) forms the same binary64 product cc * inv and the
    same constants (pw = beta exactly at step 1)"""
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    scale, n2, max_norm, clip_eps = 1024.0, 7.3e9, 2.5, 1e-6
    hs = host_state(scale, 0, n2, max_norm=max_norm, clip_eps=clip_eps, **hyper)
    inv = np.float64(1.0) / np.float64(scale)
    nrm = np.sqrt(np.float64(n2)) * inv
    r = np.float64(max_norm) / (nrm + np.float64(clip_eps))
    cc = r if r < 1.0 else np.float64(1.0)
    assert cc < 1.0 and S.fields(hs)["gm"] == float(cc * inv)
    counts, aph, nulls = TA.aligned_layout()
    _, mph, _ = TA.mixed_layout(7)
    data = TA.tensors(counts, 29, gdtype)
    coef = torch.tensor([float(cc)], dtype=torch.float64, device="cuda:0")
    for phases in (aph, mph):
        a, b = (TA.Step(counts, phases, nulls, data, gdtype, "bfloat16") for _ in range(2))
        run_dyn(a, DevState(hs))
        b.run(dict(hyper, step=1), gcoef=coef.data_ptr(), grad_mul=float(inv))
        TA.same_bits(a.results(), b.results(), "step 1")
        assert a.results()[8][0].tobytes() != data[8][0].tobytes()


@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_segments_dyn_skipped_stores_nothing(dev, gdtype):
    """skip = 1 and a gradient full of inf and NaN: p, m, v, pout and every guard
    byte keep every bit, on both bodies, segments with full tiles among them"""
    counts = [TILE + 5, 37, 3 * TILE + 21, 0, 4]
    nulls = [False, False, False, True, False]
    data = [list(d) for d in TA.tensors(counts, 23, gdtype)]
    sp = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    for d in data:
        idx = np.arange(0, d[3].size, 3)
        vals = sp[np.arange(idx.size) % 3]
        d[3][idx] = vals if gdtype == "float" else H.from_f32(vals, gdtype)
    data = [tuple(d) for d in data]
    hs = host_state(512.0, 41, INF)
    f = S.fields(hs)
    assert f["skip"] == 1.0 and f["gm"] == 0.0 and f["scale"] == 256.0 and f["step"] == 41.0
    for phases in ([(1,) * 5, (2,) * 5, (0,) * 5, (0,) * 5, (3,) * 5],
                   [(1, 2, 1, 1, 1), (0, 0, 0, 1, 0), (2, 2, 3, 2, 2), (0,) * 5, (0, 0, 0, 0, 1)]):
        s = TA.Step(counts, phases, nulls, data, gdtype, "float16")
        assert len({r[4] for r in s.plan()}) == 1 and [r[3] for r in s.plan()] == [1, 1, 4, 1]
        st = DevState(hs)
        run_dyn(s, st)
        for b in (s.p, s.m, s.v, s.o, s.g):
            assert b.unchanged()
        assert st.read().tobytes() == hs.tobytes()
        # the same launch with skip = 0 does store (the arenas are not simply out of reach)
        run_dyn(s, DevState(host_state(512.0, 41, 1.0)))
        assert not s.p.unchanged() and not s.o.unchanged()


# ---- the float16 chain over loopback ranks ---------------------------------------------------

SHARDS = TA.SHARDS
N = len(SHARDS)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
SCALING = dict(max_norm=1.0, clip_eps=1e-6, growth_factor=2.0, backoff_factor=0.5, growth_interval=3,
               min_scale=1.0, max_scale=2.0 ** 24)
SCALE0 = 65536.0
# per call: (x, planted).  Every rank's stored gradient is sign * k * 2^x with k = 1..15 and one
# sign per element on all ranks, so a float16 sum of up to four is exact while 60 * 2^x <= 65,504
# (x <= 10), and at x = 12 every rank's values are finite (15 * 4,096) while every element whose
# k sum to 16 or more overflows in the sum: the natural overflow.  The true gradient is the
# stored one / scale: with the scale between 2^13 and 2^16 and a bucket norm of some 4,000 * 2^x
# / scale, MAX_NORM = 1 clips the steps with x >= 5 and leaves those with x <= 0 alone.
CALLS = [(10, None), (0, None), (3, "inf"), (12, "natural"), (5, None), (8, "nan"), (2, None), (9, None),
         (-2, None), (7, None)]


def plan_chain(P, seed):
    """numpy only: per call the ranks' stored gradients (float16 patterns), the
    exact reduced true gradient, whether the step is skipped, and the sim's state
    after it"""
    rng = np.random.default_rng(seed)
    state = S.init(SCALE0, 0, HYPER["beta1"], HYPER["beta2"])
    calls = []
    for x, planted in CALLS:
        scale = S.fields(state)["scale"]
        per_rank, total = [[] for _ in range(P)], []
        for c in SHARDS:
            sign = rng.choice([-1.0, 1.0], P * c)
            t = np.zeros(P * c)
            for r in range(P):
                g = sign * rng.integers(1, 16, P * c) * 2.0 ** x
                per_rank[r].append(H.from_f32(g.astype(np.float32), "float16"))
                assert np.array_equal(H.to_f32(per_rank[r][-1], "float16").astype(np.float64), g)    # exact
                t = t + g
            total.append(t)
        big = max(float(np.max(np.abs(t))) for t in total if t.size)
        with np.errstate(over="ignore"):
            summed16 = [np.abs(t).astype(np.float16) for t in total]
        overflow = any(np.isinf(s).any() for s in summed16)
        if planted == "natural":
            assert overflow and 15 * 2.0 ** x <= 65504.0, "every rank finite, the sum not"
        else:
            assert not overflow and big <= 65504.0, "an unplanted overflow"
        if planted in ("inf", "nan"):
            k = 5 if planted == "inf" else 2                 # the TILE + 1 and the 5-element tensor
            per_rank[P - 1][k][SHARDS[k] // 2] = 0x7C00 if planted == "inf" else 0x7E00     # in shard 0's range
        skip = planted is not None
        n2 = INF if skip else float(sum(np.sum(t * t) for t in total))
        if planted == "nan":
            n2 = NAN
        state = S.update(state, n2, **HYPER, **SCALING)
        f = S.fields(state)
        assert f["skip"] == float(skip)
        calls.append(dict(x=x, planted=planted, scale=scale, g=per_rank, true=[t / scale for t in total],
                          skip=skip, n2=n2, state=state))
    taken = [c for c in calls if not c["skip"]]
    assert len(taken) == 7 and S.fields(state)["step"] == 7.0 and S.fields(state)["skipped"] == 3.0
    return calls


class Chain:
    def __init__(self, P, seed):
        self.P, self.cs = P, TG.comms(P)
        self.ranks = TA.Ranks(P, "float16", "float16", seed)
        rng = np.random.default_rng(seed)
        for s in self.ranks.steps:
            st = TS.fresh(SHARDS, rng, warm=False)
            for b, j in ((s.p, 0), (s.m, 1), (s.v, 2)):
                TS.load(b, [x[j] for x in st])
        # params hold the current parameters: every rank's slot = narrow(p)
        cur = [np.concatenate([A.narrow(s.p.data[k], "float16") for s in self.ranks.steps]) for k in range(N)]
        for b in self.ranks.params:
            TS.load(b, cur)
        specs = [(P * c, (k + 2) % 8, c == 0) for k, c in enumerate(SHARDS)]
        self.full = [TA.Bucket("float16", specs, [np.zeros(P * c, dtype=np.uint16) for c in SHARDS])
                     for _ in range(P)]
        self.stats = [TN.Guarded(N + 1) for _ in range(P)]
        self.states = [DevState(S.init(SCALE0, 0, HYPER["beta1"], HYPER["beta2"])) for _ in range(P)]

    def call(self, g):
        P = self.P
        for r in range(P):
            TS.load(self.full[r], g[r])
        _, st = pico_amd.loopback_reduce_scatter_multi(self.cs, "ring", [b.ptrs() for b in self.full],
                                                       self.ranks.lists("g"), "float16", "sum", shard_counts=SHARDS)
        torch.cuda.synchronize()
        assert st == [0] * P, st
        for s in self.ranks.steps:
            s.g.host = s.g.t.cpu().numpy().copy()        # what the optimizer must leave alone
        _, st = pico_amd.loopback_norm_multi(self.cs, "bine_lat", self.ranks.lists("g"), "float16",
                                             [s.ptr() for s in self.stats], counts=[SHARDS] * P)
        assert st == [0] * P, st
        for cm, stats, state in zip(self.cs, self.stats, self.states):
            pico_amd.step_update(state.ptr(), stats.ptr() + 8 * N, stream=cm.stream, **HYPER, **SCALING)
        _, st = pico_amd.loopback_adamw_multi_dyn(self.cs, "ring", [b.ptrs() for b in self.ranks.params],
                                                  self.ranks.lists("p"), self.ranks.lists("m"),
                                                  self.ranks.lists("v"), self.ranks.lists("g"),
                                                  [s.ptr() for s in self.states], gdtype="float16",
                                                  odtype="float16", shard_counts=[SHARDS] * P)
        torch.cuda.synchronize()
        assert st == [0] * P, st

    def state(self):
        """per rank, per tensor the bytes of (p, m, v); the guards and g checked"""
        return [s.results() for s in self.ranks.steps]

    def params(self):
        out = []
        for b in self.ranks.params:
            parts, guards = b.read()
            assert guards, "bytes around a parameter tensor changed"
            out.append([x.tobytes() for x in parts])
        return out


@pytest.mark.parametrize("P", [2, 4])
def test_loss_scaled_chain_skips_overflows_and_stays_within_the_float64_bounds(dev, P):
    """ten calls of reduce_scatter_multi (float16, plain sum), norm_multi,
    step_update, adamw_multi_dyn; an inf and a NaN planted on one rank and one
    natural overflow of the float16 sum: those three are skipped on every rank
    alike and change nothing but the state; the seven steps taken stay within
    optim_ref's float32 bounds of float64 AdamW on the true gradient, clipped by
    its true norm, bias-corrected by the steps taken"""
    calls = plan_chain(P, 80 + P)
    ch = Chain(P, 80 + P)
    worst, clipped = np.zeros(3), []
    for i, c in enumerate(calls):
        before, params_before = ch.state(), ch.params()
        ch.call(c["g"])
        after, params_after = ch.state(), ch.params()
        states = [s.read().tobytes() for s in ch.states]
        stats = [s.read() for s in ch.stats]
        assert all(x == states[0] for x in states), (i, "the ranks' states differ")
        assert all(x.tobytes() == stats[0].tobytes() for x in stats), (i, "the ranks' statistics differ")
        n2 = float(stats[0].view(np.float64)[N])
        if c["skip"]:
            assert not n2 <= S.DBL_MAX, (i, c["planted"], n2)
        else:
            assert n2 == c["n2"], (i, n2, c["n2"])        # integers times 4^x: exact in any order
        assert states[0] == c["state"].tobytes(), (i, S.fields(np.frombuffer(states[0], dtype=np.uint8)),
                                                   S.fields(c["state"]))
        f = S.fields(c["state"])
        if c["skip"]:
            assert f["skip"] == 1.0 and f["scale"] == c["scale"] * 0.5
            assert f["step"] == S.fields(calls[i - 1]["state"])["step"]
            for r in range(P):
                TA.same_bits(after[r], before[r], ("skipped", i, r))
            assert params_after == params_before, (i, "params changed on a skipped step")
            continue
        t = int(f["step"])
        total = float(sum(np.sum(x * x) for x in c["true"]))
        c_ref = R.clip_coef(total, SCALING["max_norm"], SCALING["clip_eps"])
        clipped.append(bool(c_ref < 1.0))
        for r in range(P):
            for k in range(N):
                ge = c["true"][k][r * SHARDS[k]:(r + 1) * SHARDS[k]] * c_ref
                assert ge.size == 0 or (2.0 ** -20 <= np.abs(ge).min() and np.abs(ge).max() <= 2.0 ** 6)
                rr = TS.within_bounds(before[r][k], after[r][k], ge, HYPER, t)
                assert (rr <= 1.0).all(), (i, t, float(c_ref), r, k, rr)
                worst = np.maximum(worst, rr)
        for r in range(P):
            for k in range(N):
                cat = b"".join(A.narrow(TS.f32(after[j][k][0]), "float16").tobytes() for j in range(P))
                assert params_after[r][k] == cat, (i, r, k)
    print(f"P = {P}: clipped {clipped}; worst |dp|, |dm|, |dv| at {worst[0]:.4g}, {worst[1]:.4g}, {worst[2]:.4g} "
          "of their bounds")
    assert True in clipped and False in clipped


def test_a_first_call_that_skips_leaves_initialised_params(dev):
    P = 2
    ch = Chain(P, 97)
    before, params_before = ch.state(), ch.params()
    want = [b"".join(A.narrow(TS.f32(before[j][k][0]), "float16").tobytes() for j in range(P)) for k in range(N)]
    assert params_before == [want] * P
    g = plan_chain(P, 97)[3]
    assert g["planted"] == "natural"
    ch.call(g["g"])
    f = pico_amd.step_state_read(ch.states[0].read())
    assert f["skip"] == 1.0 and f["step"] == 0.0 and f["skipped"] == 1.0 and f["scale"] == SCALE0 / 2
    assert ch.params() == params_before
    for r in range(P):
        TA.same_bits(ch.state()[r], before[r], ("first call", r))
