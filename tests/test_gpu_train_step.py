"""The optimizer half of a sharded training step on the GPU against AdamW and
global-norm clipping in float64 (tests/optim_ref.py, pinned to torch on the CPU
by tests/test_optim_ref.py): bine_adamw_segments over consecutive steps with the
state carried on the device, its exact symmetries, and the whole chain --
reduce-scatter, clip coefficient, AdamW plus allgather -- over loopback ranks, step by step
within the float32 error bounds and as a free-running trajectory against
torch.optim.AdamW with clip_grad_norm_."""
import numpy as np
import pytest

import adamw_sim as A
import h16_util as H
import optim_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
import test_gpu_adamw as TA  # noqa: E402  (Bucket, Step, Ranks)
import test_gpu_norm as TN  # noqa: E402  (Guarded)

TILE = TA.TILE
TYPES = TA.TYPES
COUNTS = [1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 21, 0]
NULLS = [c == 0 for c in COUNTS]
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
EDGE = dict(lr=0.1, beta1=0.0, beta2=0.5, eps=1e-3, weight_decay=0.3)
GRAD_MUL = 1.0 / 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ref_args(h):
    return h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"]


def layouts():
    """(name, phases, body): every operand on p's phase (vector body), and one
    operand in turn -- m, v, g, pout -- off it (element body)"""
    aligned = [(k % 4,) * 5 for k in range(len(COUNTS))]
    mixed = []
    for k, ph in enumerate(aligned):
        q = list(ph)
        q[1 + k % 4] = (ph[0] + 1 + k % 3) % 4
        mixed.append(tuple(q))
    return ("vector", aligned, 0), ("element", mixed, 1)


def load(b, data):
    """new contents for a Bucket's tensors, on the host image and on the device"""
    b.data = [np.ascontiguousarray(x) for x in data]
    for c, f, x in zip(b.counts, b.off, b.data):
        assert x.size == c and (c == 0 or x.dtype.itemsize == b.esz)
        b.host[f:f + c * b.esz] = x.view(np.uint8)
    b.t.copy_(torch.from_numpy(b.host))


def f32(x):
    return np.ascontiguousarray(x).view(np.float32)


def stored(g32, gdtype):
    g32 = np.ascontiguousarray(g32, dtype=np.float32)
    return g32 if gdtype == "float" else H.from_f32(g32, gdtype)


def grads(counts, rng, gdtype):
    """|g| in [2^-6, 2^15): with a coefficient in [0.25, 1] and grad_mul = 2^-10 the
    effective gradient stays in [2^-18, 2^5]"""
    return [stored(rng.choice([-1.0, 1.0], c) * rng.uniform(1.0, 2.0, c) * 2.0 ** rng.integers(-6, 15, c), gdtype)
            for c in counts]


def fresh(counts, rng, warm):
    """per tensor (p, m, v) in float32, p never zero; warm: moments of a long run,
    spread over decades, else the zero moments before step 1"""
    out = []
    for c in counts:
        p = (rng.choice([-1.0, 1.0], c) * rng.uniform(0.01, 2.0, c)).astype(np.float32)
        if warm:
            m = (rng.choice([-1.0, 1.0], c) * 10.0 ** rng.uniform(-4, 0, c)).astype(np.float32)
            v = (10.0 ** rng.uniform(-8, 0, c)).astype(np.float32)
        else:
            m, v = np.zeros(c, dtype=np.float32), np.zeros(c, dtype=np.float32)
        out.append((p, m, v))
    return out


def g_eff(g, gdtype, c, grad_mul):
    """widen(g) * c * grad_mul in float64, inside the range the bounds assume"""
    ge = A.widen(g, gdtype).astype(np.float64) * (np.float64(c) * np.float64(grad_mul))
    assert ge.size == 0 or (2.0 ** -20 <= np.abs(ge).min() and np.abs(ge).max() <= 2.0 ** 6)
    return ge


def within_bounds(before, after, ge, hyper, t):
    """the worst ratios (p, m, v) of the device's step from `before` to `after`
    (bytes of p, m, v) against the float64 step from the same state"""
    ref = R.adamw_step(f32(before[0]), f32(before[1]), f32(before[2]), ge, *ref_args(hyper), t)
    assert ref[2].size == 0 or ref[2].min() >= 2.0 ** -100
    return np.array(R.ratios([f32(x) for x in after[:3]], ref))


# ---- a. bine_adamw_segments over consecutive steps ---------------------------------------

COEFS = [0.9, 0.37, 1.0, 0.25, 0.6180339887498949, 0.5]


@pytest.mark.parametrize("t0", [0, 99999])
@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_segments_six_steps_within_the_float64_bounds(dev, gdtype, t0):
    """steps t0 + 1 .. t0 + 6 on both bodies, p, m, v carried on the device, fresh
    gradients and a new device coefficient every step, grad_mul = 1 / 1024; every
    step from the state read back before it"""
    worst = np.zeros(3)
    for name, phases, body in layouts():
        rng = np.random.default_rng(50 + body)
        st = fresh(COUNTS, rng, warm=t0 > 0)
        g = grads(COUNTS, rng, gdtype)
        s = TA.Step(COUNTS, phases, NULLS, [x + (y,) for x, y in zip(st, g)], gdtype, "bfloat16")
        assert {r[4] for r in s.plan()} == {body}, name
        coef = torch.zeros(3, dtype=torch.float64, device="cuda:0")
        for i, c in enumerate(COEFS, start=1):
            if i > 1:
                g = grads(COUNTS, rng, gdtype)
                load(s.g, g)
            coef.copy_(torch.tensor([7.0, c, 9.0], dtype=torch.float64))
            before = s.results()
            s.run(dict(HYPER, step=t0 + i), gcoef=coef.data_ptr() + 8, grad_mul=GRAD_MUL)
            after = s.results()                                  # the guards, and g unchanged
            for k in range(len(COUNTS)):
                r = within_bounds(before[k], after[k], g_eff(g[k], gdtype, c, GRAD_MUL), HYPER, t0 + i)
                assert (r <= 1.0).all(), (name, t0 + i, k, COUNTS[k], r)
                worst = np.maximum(worst, r)
                assert after[k][3].tobytes() == A.narrow(f32(after[k][0]), "bfloat16").tobytes(), (name, i, k)
                if COUNTS[k]:
                    assert after[k][0].tobytes() != before[k][0].tobytes()
            assert coef.cpu().numpy().tolist() == [7.0, c, 9.0]
    print(f"{gdtype}, t0 = {t0}: worst |dp|, |dm|, |dv| at {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} "
          "of their bounds")


# ---- b. properties that need no reference ------------------------------------------------

def prop_data(gdtype, seed):
    rng = np.random.default_rng(seed)
    return [x + (y,) for x, y in zip(fresh(COUNTS, rng, warm=True), grads(COUNTS, rng, gdtype))]


def run_once(phases, body, data, gdtype, hyper, gcoef=None, grad_mul=1.0):
    s = TA.Step(COUNTS, phases, NULLS, data, gdtype, "bfloat16")
    assert {r[4] for r in s.plan()} == {body}
    s.run(hyper, gcoef=gcoef, grad_mul=grad_mul)
    return s.results()


def negated(x, dtype):
    if dtype == "float":
        return -np.ascontiguousarray(x, dtype=np.float32)
    return np.ascontiguousarray(x, dtype=np.uint16) ^ np.uint16(0x8000)


@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_segments_exact_properties(dev, gdtype):
    data = prop_data(gdtype, 60)
    live = [k for k, c in enumerate(COUNTS) if c]
    zero_g = np.float32 if gdtype == "float" else np.uint16
    for name, phases, body in layouts():
        # 1. lr = 0: p keeps its bits, m and v move
        got = run_once(phases, body, data, gdtype, dict(HYPER, lr=0.0, step=3), grad_mul=GRAD_MUL)
        for k in live:
            p, m, v, _ = data[k]
            assert got[k][0].tobytes() == p.tobytes(), (name, "lr = 0", k)
            assert got[k][1].tobytes() != m.tobytes() and got[k][2].tobytes() != v.tobytes()
        # 2. g = 0 and m = 0: the decay alone
        still = [(p, np.zeros_like(m), v, np.zeros(g.size, dtype=zero_g)) for p, m, v, g in data]
        got = run_once(phases, body, still, gdtype, dict(EDGE, step=5))
        dk = np.float64(np.float32(1.0 - EDGE["lr"] * EDGE["weight_decay"]))
        b2 = np.float64(np.float32(EDGE["beta2"]))
        for k in live:
            p, _, v, _ = data[k]
            assert got[k][0].tobytes() == (p.astype(np.float64) * dk).astype(np.float32).tobytes(), (name, "p dk", k)
            assert not got[k][1].any(), (name, "m' = 0", k)
            assert got[k][2].tobytes() == (v.astype(np.float64) * b2).astype(np.float32).tobytes(), (name, "v b2", k)
        # 3. p, m, g negated: p', m' negated, v' the same
        hyper = dict(HYPER, step=7)
        pos = run_once(phases, body, data, gdtype, hyper, grad_mul=GRAD_MUL)
        neg = run_once(phases, body, [(-p, -m, v, negated(g, gdtype)) for p, m, v, g in data], gdtype, hyper,
                       grad_mul=GRAD_MUL)
        for k in live:
            assert neg[k][0].tobytes() == (-f32(pos[k][0])).tobytes(), (name, "-p", k)
            assert neg[k][1].tobytes() == (-f32(pos[k][1])).tobytes(), (name, "-m", k)
            assert neg[k][2].tobytes() == pos[k][2].tobytes(), (name, "v", k)
            assert neg[k][3].tobytes() == negated(pos[k][3].view(np.uint16), "bfloat16").tobytes(), (name, "-pout", k)
        # 4. a device coefficient c and a host factor s with an exact product: the host factor c * s alone
        c, sc = 0.375, 2.0 ** -7
        coef = torch.tensor([c], dtype=torch.float64, device="cuda:0")
        a = run_once(phases, body, data, gdtype, hyper, gcoef=coef.data_ptr(), grad_mul=sc)
        b = run_once(phases, body, data, gdtype, hyper, grad_mul=c * sc)
        TA.same_bits(a, b, (name, "c * s"))
        assert any(a[k][0].tobytes() != pos[k][0].tobytes() for k in live)      # the factor matters


# ---- c, d. the whole step over loopback ranks ----------------------------------------------

SHARDS = TA.SHARDS
assert SHARDS == [0, 1, 5, 1023, TILE, TILE + 1, 2 * TILE + 21, 4]
N = len(SHARDS)
# (gradient type, reduce-scatter op, wide, the optimizer's grad_mul as a function of P)
ROWS = {"bfloat16": ("avg", True, lambda P: 1.0), "float": ("sum", False, lambda P: 1.0 / P)}
MAX_NORM, CLIP_EPS = 1.0, 1e-6
# the step's power of two: the reduced bucket's norm lies between 500 * 2^e (the mean of two
# ranks, magnitudes up to 4) and 12,500 * 2^e (the sum of four, up to 15), so with MAX_NORM = 1
# e <= -14 leaves the gradient alone and e >= -9 clips it
EXPS = [-14, -3, -9, -15, 2, -6, -13, 0]


class Chain:
    """P loopback ranks with their shards of p, m, v, g (tests/test_gpu_adamw.py's
    Ranks, 16-bit parameters), every rank's full gradient tensors and statistics"""

    def __init__(self, P, gdtype, seed):
        self.P, self.gdtype = P, gdtype
        self.op, self.wide, gm = ROWS[gdtype]
        self.grad_mul = gm(P)
        self.cs = TG.comms(P)
        self.rng = np.random.default_rng(seed)
        self.ranks = TA.Ranks(P, gdtype, "bfloat16", seed)
        self.p0 = []
        for s in self.ranks.steps:
            st = fresh(SHARDS, self.rng, warm=False)
            self.p0.append([x[0] for x in st])
            for b, j in ((s.p, 0), (s.m, 1), (s.v, 2)):
                load(b, [x[j] for x in st])
        per = 16 // TA.ESZ[gdtype]
        specs = [(P * c, (k + 2) % per, c == 0) for k, c in enumerate(SHARDS)]
        empty = np.float32 if gdtype == "float" else np.uint16
        self.full = [TA.Bucket(gdtype, specs, [np.zeros(P * c, dtype=empty) for c in SHARDS]) for _ in range(P)]
        self.stats = [TN.Guarded(N + 2) for _ in range(P)]

    def shard(self, x, k, j):
        return x[j * SHARDS[k]:(j + 1) * SHARDS[k]]

    def new_gradients(self, e, lo, hi, unit):
        """per rank and tensor: integers in [lo, hi] times unit * 2^e, one sign per
        element on every rank; returns the exact float64 sum over the ranks"""
        total = []
        per_rank = [[] for _ in range(self.P)]
        for c in SHARDS:
            sign = self.rng.choice([-1.0, 1.0], self.P * c)
            t = np.zeros(self.P * c)
            for r in range(self.P):
                x = sign * self.rng.integers(lo, hi + 1, self.P * c) * unit * 2.0 ** e
                per_rank[r].append(x)
                t = t + x
            total.append(t)
        for r in range(self.P):
            load(self.full[r], [stored(x, self.gdtype) for x in per_rank[r]])
            for x, y in zip(per_rank[r], self.full[r].data):
                assert np.array_equal(A.widen(y, self.gdtype).astype(np.float64), x)   # exact in the type
        return total

    def reduce_scatter(self, total):
        """the ranks' g shards = the exact mean (avg) or sum; returns those tensors"""
        _, st = pico_amd.loopback_reduce_scatter_multi(self.cs, "ring", [b.ptrs() for b in self.full],
                                                       self.ranks.lists("g"), self.gdtype, self.op,
                                                       shard_counts=SHARDS, wide=self.wide)
        torch.cuda.synchronize()
        assert st == [0] * self.P, st
        want = [t / self.P if self.op == "avg" else t for t in total]
        for r, s in enumerate(self.ranks.steps):
            parts, guards = s.g.read()
            assert guards and self.full[r].unchanged()
            for k in range(N):
                got = A.widen(parts[k].view(np.float32 if self.gdtype == "float" else np.uint16), self.gdtype)
                assert np.array_equal(got.astype(np.float64), self.shard(want[k], k, r)), ("reduce-scatter", r, k)
            s.g.host = s.g.t.cpu().numpy().copy()        # what the next call finds
        return want

    def coefficient(self):
        """loopback_clip_multi(scale=False): the statistics and the clip coefficient
        into every rank's stats, the shards left as the reduce-scatter wrote them"""
        _, st = pico_amd.loopback_clip_multi(self.cs, "bine_lat", self.ranks.lists("g"), self.gdtype, MAX_NORM,
                                             CLIP_EPS, [s.ptr() for s in self.stats], counts=[SHARDS] * self.P,
                                             scale=False)
        torch.cuda.synchronize()
        assert st == [0] * self.P, st
        assert all(s.g.unchanged() for s in self.ranks.steps), "the coefficient alone changed a gradient"
        return [s.read() for s in self.stats]

    def adamw(self, hyper, t):
        gc = [s.ptr() + 8 * (N + 1) for s in self.stats]
        _, st = pico_amd.loopback_adamw_multi(self.cs, "ring", [b.ptrs() for b in self.ranks.params],
                                              self.ranks.lists("p"), self.ranks.lists("m"), self.ranks.lists("v"),
                                              self.ranks.lists("g"), gcoef=gc, grad_mul=self.grad_mul,
                                              gdtype=self.gdtype, odtype="bfloat16", shard_counts=[SHARDS] * self.P,
                                              step=t, **hyper)
        torch.cuda.synchronize()
        assert st == [0] * self.P, st

    def state(self):
        """per rank, per tensor the bytes of (p, m, v); the guards and g checked"""
        return [s.results() for s in self.ranks.steps]


def chain_steps(P, gdtype, nsteps=6):
    ch = Chain(P, gdtype, 70 + P)
    worst, clipped = np.zeros(3), []
    for t, e in enumerate(EXPS[:nsteps], start=1):
        total = ch.new_gradients(e, 1, 15, 1.0)
        reduced = ch.reduce_scatter(total)
        stats = ch.coefficient()
        # the statistics: every square is an integer times 4^e, so the sums are exact in any order
        want = [float(np.sum(x * x)) for x in reduced]
        s0 = stats[0].view(np.float64)
        assert s0[:N].tolist() == want and s0[N] == float(sum(want)), (t, "sum of squares")
        assert abs(s0[N] - sum(want)) <= sum(SHARDS) * P * 2.0 ** -52 * sum(want)
        c_ref = R.clip_coef(sum(want), MAX_NORM, CLIP_EPS)
        for r in range(P):
            assert stats[r].tobytes() == stats[0].tobytes(), (t, r, "statistics differ between the ranks")
        assert abs(s0[N + 1] - c_ref) <= 4 * np.spacing(c_ref), (t, s0[N + 1], c_ref)
        clipped.append(bool(c_ref < 1.0))
        before = ch.state()
        ch.adamw(HYPER, t)
        after = ch.state()                                   # asserts the gradient shards unchanged
        # textbook: the reduced gradient, clipped to MAX_NORM by its global norm, times grad_mul
        for r in range(P):
            for k in range(N):
                ge = ch.shard(reduced[k], k, r) * (c_ref * ch.grad_mul)
                assert ge.size == 0 or (2.0 ** -20 <= np.abs(ge).min() and np.abs(ge).max() <= 2.0 ** 6)
                rr = within_bounds(before[r][k], after[r][k], ge, HYPER, t)
                assert (rr <= 1.0).all(), (t, e, float(c_ref), r, k, rr)
                worst = np.maximum(worst, rr)
        # every rank's parameters: the owners' narrow(p') one after another
        for r in range(P):
            got, guards = ch.ranks.params[r].read()
            assert guards, "bytes around a parameter tensor changed"
            for k in range(N):
                cat = b"".join(A.narrow(f32(after[j][k][0]), "bfloat16").tobytes() for j in range(P))
                assert got[k].tobytes() == cat, (t, r, k)
    print(f"P = {P}, {gdtype}: clipped {clipped}; worst |dp|, |dm|, |dv| at "
          f"{worst[0]:.4g}, {worst[1]:.4g}, {worst[2]:.4g} of their bounds")
    assert True in clipped and False in clipped


@pytest.mark.parametrize("gdtype", sorted(ROWS))
@pytest.mark.parametrize("P", [2, 4])
def test_train_step_chain_within_the_float64_bounds(dev, P, gdtype):
    """reduce_scatter_multi, clip_multi, adamw_multi with gcoef = &stats[n + 1], in
    that order on the one set of gradient shards, six steps, against the float64
    step on the unsharded tensors.  clip_multi runs with scale=False, the
    coefficient alone: adamw_multi applies it, and the shards must reach it
    unscaled."""
    chain_steps(P, gdtype)


def trajectory(gdtype):
    """8 free-running steps at P = 2; returns (D32, the device's deviation)"""
    P = 2
    ch = Chain(P, gdtype, 90)
    live = [k for k, c in enumerate(SHARDS) if c]
    full_p0 = [np.concatenate([ch.p0[j][k] for j in range(P)]) for k in live]
    runs = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.from_numpy(x.astype(np.float64)).to(dt).requires_grad_(True) for x in full_p0]
        runs[dt] = (ps, torch.optim.AdamW(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]),
                                          eps=HYPER["eps"], weight_decay=HYPER["weight_decay"], foreach=False))
    clipped = []
    for t, e in enumerate(EXPS, start=1):
        total = ch.new_gradients(e, 1, 16, 0.25)             # magnitudes in [0.25, 4] * 2^e
        reduced = ch.reduce_scatter(total)
        stats = ch.coefficient()
        clipped.append(bool(stats[0].view(np.float64)[N + 1] < 1.0))
        ch.adamw(HYPER, t)
        for dt, (ps, opt) in runs.items():
            for x, k in zip(ps, live):
                x.grad = torch.tensor(reduced[k], dtype=dt)                  # a copy: the clip is in place
                assert np.array_equal(x.grad.numpy().astype(np.float64), reduced[k])     # exact in float32 too
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)      # its eps is 1e-6, CLIP_EPS
            for x in ps:
                x.grad.mul_(ch.grad_mul)                                     # 1 or 1 / P: exact
            opt.step()
    assert True in clipped and False in clipped
    state = ch.state()
    dev_p = [np.concatenate([f32(state[j][k][0]) for j in range(P)]).astype(np.float64) for k in live]
    p64 = [x.detach().numpy() for x in runs[torch.float64][0]]
    p32 = [x.detach().numpy().astype(np.float64) for x in runs[torch.float32][0]]
    d32 = max(float(np.max(np.abs(a - b))) for a, b in zip(p32, p64))
    ddev = max(float(np.max(np.abs(a - b))) for a, b in zip(dev_p, p64))
    moved = max(float(np.max(np.abs(a - b.astype(np.float64)))) for a, b in zip(p64, full_p0))
    print(f"{gdtype}: D32 = {d32:.3e}, device deviation = {ddev:.3e}, p moved by {moved:.3e}")
    assert moved > 1e-3 and d32 > 0
    return d32, ddev


@pytest.mark.parametrize("gdtype", sorted(ROWS))
def test_train_step_trajectory_against_torch(dev, gdtype):
    """the chain of the test above, eight steps never resynchronised: the final p
    against float64 torch.optim.AdamW with clip_grad_norm_, no further from it
    than 4 times what torch's own float32 AdamW is (D32)"""
    d32, ddev = trajectory(gdtype)
    assert ddev <= 4 * d32, (ddev, d32)


def test_clip_multi_coefficient_alone(dev):
    """loopback_clip_multi(scale=False) writes the statistics and the coefficient
    of the scaling call, bit for bit, and leaves every tensor alone; a negative
    max_norm is refused before anything runs"""
    P = 2
    cs = TG.comms(P)
    for dtype, max_norm in (("float", 7.5), ("bfloat16", 1e9)):
        a, b = TN.rank_buckets(dtype, P, 42), TN.rank_buckets(dtype, P, 42)
        n = len(a[0].counts)
        sa, sb = [TN.Guarded(n + 2) for _ in range(P)], [TN.Guarded(n + 2) for _ in range(P)]
        for bs, stats, scale in ((a, sa, True), (b, sb, False)):
            _, st = pico_amd.loopback_clip_multi(cs, "bine_lat", [x.ptrs() for x in bs], dtype, max_norm, 1e-6,
                                                 [s.ptr() for s in stats], counts=[x.counts for x in bs], scale=scale)
            torch.cuda.synchronize()
            assert st == [0] * P
        for r in range(P):
            assert sa[r].read().tobytes() == sb[r].read().tobytes(), (dtype, r)
            assert b[r].unchanged()
        c = sb[0].read().view(np.float64)[n + 1]
        assert (c < 1.0) == (dtype == "float") and any(not x.unchanged() for x in a) == (c < 1.0)
    fresh_stats = [TN.Guarded(n + 2) for _ in range(P)]
    with pytest.raises(pico_amd.BineError) as ei:
        pico_amd.loopback_clip_multi(cs, "bine_lat", [x.ptrs() for x in b], "bfloat16", -1.0, 0.0,
                                     [s.ptr() for s in fresh_stats], counts=[x.counts for x in b], scale=False)
    assert ei.value.status == 1
    torch.cuda.synchronize()
    assert all((s.read() == TN.Guarded.PAT).all() for s in fresh_stats)
