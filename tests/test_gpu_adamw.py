"""Fused AdamW step on the GPU: bine_adamw_segments (k_adamw_segs) against
adamw_sim, the numpy float32 statement of the header's contract, bit for bit on
both bodies, and bine_adamw_multi over loopback ranks against the sim and
against its two parts called separately.  (Real processes and graph mode:
tools/adamw_check.py, tests/test_gpu_adamw_rccl.py.)"""
import numpy as np
import pytest

import adamw_sim as A
import h16_util as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402

S = _lib.ADAMW_SEGS_PER_LAUNCH
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
GUARD = 0xA5
TILE = 8192
COUNTS = [0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 21]
HYPERS = [dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1),
          dict(lr=3e-2, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.0, step=1000)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Bucket:
    """tensors (count, phase in elements, null) in one arena of guard bytes, each
    with 16 guard bytes or more on either side; null: an empty tensor passed as
    NULL (tests/test_gpu_norm.py's helper)"""

    def __init__(self, dtype, specs, data):
        self.dtype, self.esz, self.specs = dtype, ESZ[dtype], specs
        self.data = [np.ascontiguousarray(x) for x in data]
        self.off, o = [], 0
        for c, ph, _ in specs:
            self.off.append(o + 16 + ph * self.esz)
            o = (o + 16 + ph * self.esz + c * self.esz + 16 + 15) & ~15
        self.host = np.full(o + 16, GUARD, dtype=np.uint8)
        for (c, _, _), f, x in zip(specs, self.off, self.data):
            assert x.size == c
            self.host[f:f + c * self.esz] = x.view(np.uint8)
        self.t = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0
        self.counts = [c for c, _, _ in specs]

    def ptrs(self):
        return [None if null else self.t.data_ptr() + f for (_, _, null), f in zip(self.specs, self.off)]

    def unchanged(self):
        return bool(np.array_equal(self.t.cpu().numpy(), self.host))

    def read(self):
        """(the tensors' bytes, whether every other byte is as it was)"""
        got = self.t.cpu().numpy()
        mask = np.zeros(got.size, dtype=bool)
        parts = []
        for c, f in zip(self.counts, self.off):
            mask[f:f + c * self.esz] = True
            parts.append(got[f:f + c * self.esz].copy())
        return parts, bool(np.array_equal(got[~mask], self.host[~mask]))


# ---- inputs --------------------------------------------------------------------------------

def _sprinkle(x, rng, patterns):
    """every 11th element or so replaced by one of the float32 bit patterns"""
    if x.size:
        idx = rng.random(x.size) < 0.09
        x.view(np.uint32)[idx] = rng.choice(np.array(patterns, dtype=np.uint32), int(idx.sum()))
    return x


def tensors(counts, seed, gdtype):
    """per tensor (p, m, v, g): finite, v >= 0; g, m and v with subnormals, v with
    zeros, all of them with +-0 (eps > 0 in every case here, so v = 0 is defined)"""
    rng = np.random.default_rng(seed)
    sub = [1, 0x7FFFFF, 0x400000, 0x12345]
    out = []
    for c in counts:
        p = _sprinkle(rng.standard_normal(c).astype(np.float32), rng, [0, 0x80000000])
        m = _sprinkle((0.1 * rng.standard_normal(c)).astype(np.float32), rng,
                      [0, 0x80000000] + sub + [s | 0x80000000 for s in sub])
        v = _sprinkle(((0.1 * rng.standard_normal(c)) ** 2).astype(np.float32), rng, [0, 0, 0] + sub)
        g = rng.standard_normal(c).astype(np.float32)
        if gdtype == "float":
            g = _sprinkle(g, rng, [0, 0x80000000] + sub + [s | 0x80000000 for s in sub])
        else:
            g = H.from_f32(g, gdtype)
            idx = rng.random(c) < 0.09         # 16-bit subnormals and zeros of both signs
            g[idx] = rng.choice(np.array([0, 0x8000, 1, 0x8001, 0x7F, 0x807F, 0x3F], dtype=np.uint16), int(idx.sum()))
        assert np.isfinite(p).all() and np.isfinite(m).all() and (v >= 0).all()
        out.append((p, m, v, g))
    return out


class Step:
    """the five arenas of one call; phases: per tensor (p, m, v, g, pout) in elements"""

    def __init__(self, counts, phases, nulls, data, gdtype, odtype):
        self.counts, self.gdtype, self.odtype, self.data = counts, gdtype, odtype, data
        spec = lambda j: [(c, ph[j], nl) for c, ph, nl in zip(counts, phases, nulls)]  # noqa: E731
        self.p = Bucket("float", spec(0), [d[0] for d in data])
        self.m = Bucket("float", spec(1), [d[1] for d in data])
        self.v = Bucket("float", spec(2), [d[2] for d in data])
        self.g = Bucket(gdtype, spec(3), [d[3] for d in data])
        self.o = None
        if odtype is not None:
            self.o = Bucket(odtype, spec(4), [np.zeros(c, dtype=np.float32 if odtype == "float" else np.uint16)
                                              for c in counts])

    def plan(self):
        z = lambda b: [x or 0 for x in b.ptrs()]  # noqa: E731
        return pico_amd.plan_adamw(z(self.p), z(self.m), z(self.v), z(self.g), None if self.o is None else z(self.o),
                                   self.counts, self.gdtype, self.odtype or "float")

    def run(self, hyper, gcoef=None, grad_mul=1.0):
        pico_amd.adamw_segments(self.p.ptrs(), self.m.ptrs(), self.v.ptrs(), self.g.ptrs(),
                                None if self.o is None else self.o.ptrs(), gcoef=gcoef, grad_mul=grad_mul,
                                gdtype=self.gdtype, odtype=self.odtype or "float", counts=self.counts, **hyper)
        torch.cuda.synchronize()

    def results(self):
        """per tensor the bytes of (p', m', v', pout); the guards and g checked"""
        out = []
        for b in (self.p, self.m, self.v) + ((self.o,) if self.o is not None else ()):
            parts, guards = b.read()
            assert guards, "bytes around a tensor changed"
            out.append(parts)
        assert self.g.unchanged(), "the gradient or the bytes around it changed"
        return list(zip(*out))


def sim_results(data, gdtype, odtype, hyper, gm=A.GM_ONE):
    consts = pico_amd.adamw_consts(**hyper)
    out = []
    for p, m, v, g in data:
        p2, m1, v1 = A.step(p, m, v, g, gdtype, consts, gm)
        r = [p2, m1, v1] + ([A.narrow(p2, odtype)] if odtype is not None else [])
        out.append(tuple(x.view(np.uint8) for x in r))
    return out


def same_bits(got, want, what):
    assert len(got) == len(want)
    for k, (gk, wk) in enumerate(zip(got, want)):
        for name, a, b in zip(("p", "m", "v", "pout"), gk, wk):
            assert a.tobytes() == b.tobytes(), (what, k, name, a.size)


def aligned_layout():
    """every count at every element phase of p, every operand congruent with p;
    a NULL empty and a non-NULL empty among them"""
    counts, phases, nulls = [], [], []
    for ph in range(4):
        for c in COUNTS:
            counts.append(c), phases.append((ph,) * 5), nulls.append(c == 0 and ph % 2 == 1)
    return counts, phases, nulls


def mixed_layout(seed):
    """the same counts, one operand (in turn m, v, g, pout) off p's phase"""
    rng = np.random.default_rng(seed)
    counts, phases, nulls = aligned_layout()
    mixed = []
    for k, ph in enumerate(phases):
        q = list(ph)
        q[1 + k % 4] = (ph[0] + 1 + int(rng.integers(0, 3))) % 4
        mixed.append(tuple(q))
    return counts, mixed, nulls


OUT_TYPES = TYPES + [None]


@pytest.mark.parametrize("odtype", OUT_TYPES, ids=lambda t: t or "absent")
@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_segments_is_the_sim_on_both_bodies(dev, gdtype, odtype):
    """p', m', v' and pout bit for bit adamw_sim's on the vector body (aligned
    phases) and on the element body (mixed phases), so the two bodies agree on
    the same values; guard bytes and g untouched; steps 1 and 1,000, weight
    decay 0.01 and 0; gcoef = NULL and grad_mul = 1.0: gm = 1"""
    counts, aph, nulls = aligned_layout()
    _, mph, _ = mixed_layout(3)
    data = tensors(counts, 11, gdtype)
    for hyper in HYPERS:
        want = sim_results(data, gdtype, odtype, hyper)
        for name, phases, body in (("vector", aph, 0), ("element", mph, 1)):
            s = Step(counts, phases, nulls, data, gdtype, odtype)
            bodies = {r[4] for r in s.plan()}
            if name == "element" and odtype is None:
                # with no pout a tensor whose pout alone is off p's phase is aligned
                assert bodies == {0, 1}
            else:
                assert bodies == {body}, (name, bodies)
            s.run(hyper)
            same_bits(s.results(), want, (name, hyper["step"]))


@pytest.mark.parametrize("gdtype", ["float", "bfloat16"])
def test_adamw_gcoef_is_read_from_the_device(dev, gdtype):
    """gcoef -> 0.37 on the device and grad_mul = 1 / 1024: gm = float32(0.37 * 2^-10)"""
    counts, aph, nulls = aligned_layout()
    _, mph, _ = mixed_layout(5)
    data = tensors(counts, 13, gdtype)
    coef = torch.from_numpy(np.array([7.0, 0.37, 9.0], dtype=np.float64)).to("cuda:0")
    gm = np.float32(np.float64(0.37) * np.float64(2.0 ** -10))
    assert A.gm_of(0.37, 1.0 / 1024).tobytes() == gm.tobytes()
    want = sim_results(data, gdtype, "bfloat16", HYPERS[0], gm)
    for phases in (aph, mph):
        s = Step(counts, phases, nulls, data, gdtype, "bfloat16")
        s.run(HYPERS[0], gcoef=coef.data_ptr() + 8, grad_mul=1.0 / 1024)
        same_bits(s.results(), want, "gcoef")
    assert coef.cpu().numpy().tolist() == [7.0, 0.37, 9.0]
    # the coefficient matters: gm = 1 gives other bits
    assert sim_results(data, gdtype, "bfloat16", HYPERS[0])[8][0].tobytes() != want[8][0].tobytes()


def test_adamw_many_segments_equal_per_tensor_calls(dev):
    """2 * 64 + 37 non-empty tensors, empties in between: three launches"""
    rng = np.random.default_rng(17)
    counts, phases, nulls = [], [], []
    for k in range(2 * S + 37):
        ph = int(rng.integers(0, 4))
        q = [ph] * 5
        if k % 3 == 0:
            q[1 + int(rng.integers(0, 4))] = (ph + 1) % 4
        counts.append(int(rng.choice([1, 3, 4, 5, 100, 1025])))
        phases.append(tuple(q)), nulls.append(False)
        if k % 5 == 0:
            counts.append(0), phases.append((0,) * 5), nulls.append(k % 10 == 0)
    data = tensors(counts, 19, "float16")
    s = Step(counts, phases, nulls, data, "float16", "bfloat16")
    plan = s.plan()
    assert [r[0] for r in plan] == [j // S for j in range(2 * S + 37)] and {r[4] for r in plan} == {0, 1}
    s.run(HYPERS[1])
    got = s.results()
    same_bits(got, sim_results(data, "float16", "bfloat16", HYPERS[1]), "many")
    one = Step(counts, phases, nulls, data, "float16", "bfloat16")
    for k, c in enumerate(counts):                       # one call per tensor on a second copy
        if c:
            pico_amd.adamw_segments([one.p.ptrs()[k]], [one.m.ptrs()[k]], [one.v.ptrs()[k]], [one.g.ptrs()[k]],
                                    [one.o.ptrs()[k]], gdtype="float16", odtype="bfloat16", counts=[c], **HYPERS[1])
    torch.cuda.synchronize()
    same_bits(got, one.results(), "per tensor")


def nan_same(got, want, dtype):
    """bit-equal where want is not NaN, NaN where it is"""
    if dtype == "float":
        g, w = got.view(np.float32), want.view(np.float32)
        nan = np.isnan(w)
        return bool(np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32)) and np.isnan(g[nan]).all())
    return H.same(got.view(np.uint16), want.view(np.uint16), dtype)


@pytest.mark.parametrize("gdtype", TYPES)
def test_adamw_specials_follow_ieee(dev, gdtype):
    """NaN and +-inf in g: nothing is skipped or clamped"""
    counts = [TILE + 5, 37]
    data = [list(d) for d in tensors(counts, 23, gdtype)]
    sp = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    for d in data:
        idx = np.arange(0, d[3].size, 7)
        vals = sp[np.arange(idx.size) % 3]
        d[3][idx] = vals if gdtype == "float" else H.from_f32(vals, gdtype)
    data = [tuple(d) for d in data]
    odtype = "float16"
    want = sim_results(data, gdtype, odtype, HYPERS[0])
    assert np.isnan(want[0][0].view(np.float32)).any() and np.isinf(want[0][2].view(np.float32)).any()
    for phases in ([(1,) * 5, (2,) * 5], [(1, 2, 1, 1, 1), (0, 0, 0, 1, 0)]):
        s = Step(counts, phases, [False, False], data, gdtype, odtype)
        s.run(HYPERS[0])
        for k, (gk, wk) in enumerate(zip(s.results(), want)):
            for name, a, b, t in zip("pmvo", gk, wk, ("float", "float", "float", odtype)):
                assert nan_same(a, b, t), (k, name)


# ---- the collective over loopback ranks ----------------------------------------------------

SHARDS = [0, 1, 5, 1023, TILE, TILE + 1, 2 * TILE + 21, 4]


class Ranks:
    """per rank: its shards' Step (aligned phases; pout unused) and the full
    parameter tensors, params[k] = P * SHARDS[k] elements of odtype"""

    def __init__(self, P, gdtype, odtype, seed):
        self.P, self.gdtype, self.odtype, self.n = P, gdtype, odtype, len(SHARDS)
        self.data = [tensors(SHARDS, seed + r, gdtype) for r in range(P)]
        ph = [((k + 1) % 4,) * 5 for k in range(self.n)]
        nulls = [c == 0 for c in SHARDS]
        self.steps = [Step(SHARDS, ph, nulls, self.data[r], gdtype, None) for r in range(P)]
        specs = [(P * c, (k + 1) % (16 // ESZ[odtype]), c == 0) for k, c in enumerate(SHARDS)]
        fill = np.float32 if odtype == "float" else np.uint16
        self.params = [Bucket(odtype, specs, [np.full(P * c, 7, dtype=fill) for c in SHARDS]) for _ in range(P)]

    def lists(self, which):
        return [getattr(s, which).ptrs() for s in self.steps]

    def multi(self, cs, algo, hyper, g=None, gcoef=None):
        _, st = pico_amd.loopback_adamw_multi(cs, algo, [b.ptrs() for b in self.params], self.lists("p"),
                                              self.lists("m"), self.lists("v"), g or self.lists("g"), gcoef=gcoef,
                                              gdtype=self.gdtype, odtype=self.odtype,
                                              shard_counts=[SHARDS] * self.P, **hyper)
        torch.cuda.synchronize()
        assert st == [0] * self.P, st

    def state(self):
        """per rank the bytes of (params, p, m, v) arenas"""
        return [[b.t.cpu().numpy().tobytes() for b in (self.params[r], s.p, s.m, s.v)]
                for r, s in enumerate(self.steps)]


@pytest.mark.parametrize("P", [2, 4])
def test_adamw_multi_is_the_sim_and_its_two_parts(dev, P):
    cs = TG.comms(P)
    for gdtype, odtype, algo in (("bfloat16", "bfloat16", "ring"), ("float", "float16", "recursivedoubling")):
        hyper = HYPERS[P % 2]
        fused, parts = Ranks(P, gdtype, odtype, 31), Ranks(P, gdtype, odtype, 31)
        fused.multi(cs, algo, hyper)
        # every rank's params: the concatenation of all ranks' narrow(p') from the sim
        sims = [sim_results(fused.data[r], gdtype, odtype, hyper) for r in range(P)]
        for r in range(P):
            got, guards = fused.params[r].read()
            assert guards, "bytes around a parameter tensor changed"
            for k in range(fused.n):
                want = b"".join(sims[j][k][3].tobytes() for j in range(P))
                assert got[k].tobytes() == want, (gdtype, r, k)
            same_bits(fused.steps[r].results(), [x[:3] for x in sims[r]], ("shards", r))
        # adamw_segments + loopback_allgather_multi called separately
        for r, s in enumerate(parts.steps):
            slot = [None if c == 0 else a + r * c * ESZ[odtype] for a, c in zip(parts.params[r].ptrs(), SHARDS)]
            pico_amd.adamw_segments(s.p.ptrs(), s.m.ptrs(), s.v.ptrs(), s.g.ptrs(), slot, gdtype=gdtype,
                                    odtype=odtype, counts=SHARDS, **hyper)
        torch.cuda.synchronize()
        _, st = pico_amd.loopback_allgather_multi(cs, algo, None, [b.ptrs() for b in parts.params], odtype,
                                                  shard_counts=SHARDS)
        torch.cuda.synchronize()
        assert st == [0] * P
        assert fused.state() == parts.state(), (gdtype, odtype)


@pytest.mark.parametrize("P", [2, 4])
def test_adamw_multi_after_clip_multi(dev, P):
    """gcoef = &stats[n + 1] of loopback_clip_multi against clip_segments on a
    copy of g followed by the call with gcoef = NULL.  For gdtype float only: the
    clipped float gradient g * (float)c times gm = 1 is the fused call's g *
    (float)(c * 1.0).  For the 16-bit types the fused form skips the rounding of
    the clipped gradient to 16 bits by design, so the two differ there."""
    cs = TG.comms(P)
    algo = "ring"
    fused, ref = Ranks(P, "float", "bfloat16", 41), Ranks(P, "float", "bfloat16", 41)
    n = fused.n
    stats = [torch.zeros(n + 2, dtype=torch.float64, device="cuda:0") for _ in range(P)]
    # the clip runs on ref's gradients (scaled in place); fused keeps the unclipped ones
    _, st = pico_amd.loopback_clip_multi(cs, "bine_lat", ref.lists("g"), "float", 3.0, 1e-6,
                                         [s.data_ptr() for s in stats], counts=[SHARDS] * P)
    torch.cuda.synchronize()
    assert st == [0] * P
    c = [float(s[n + 1].item()) for s in stats]
    assert 0.0 < c[0] < 1.0 and c == [c[0]] * P
    assert not any(s.g.unchanged() for s in ref.steps)
    fused.multi(cs, algo, HYPERS[0], gcoef=[s.data_ptr() + 8 * (n + 1) for s in stats])
    ref.multi(cs, algo, HYPERS[0])
    assert fused.state() == ref.state()
    assert all(s.g.unchanged() for s in fused.steps)
