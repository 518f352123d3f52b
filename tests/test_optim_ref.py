"""tests/optim_ref.py, the float64 AdamW and clipping reference, pinned to an
implementation nobody here wrote (torch.optim.AdamW and clip_grad_norm_ on the
CPU in float64), and its float32 error bounds shown to hold for the numpy
float32 statement of bine_adamw_segments (tests/adamw_sim.py with the constants
of bine_adamw_consts) and to reject the classic formula errors.  No GPU."""
import numpy as np
import pytest

import adamw_sim as A
import h16_util as H
import optim_ref as R

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402

HYPERS = [dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01),
          dict(lr=3e-2, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.0),
          dict(lr=0.1, beta1=0.0, beta2=0.5, eps=1e-3, weight_decay=0.3)]
IDS = ["default", "fast", "edge"]
TYPES = ["bfloat16", "float", "float16"]
STEPS = [1, 2, 10, 1000, 10 ** 6]
N = 20000


def ref_args(h):
    return h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"]


# ---- the reference against torch ---------------------------------------------------------

def rel(a, b):
    """the worst |a - b| / |b| (0 where both are 0)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
    return float(r.max())


LIMIT = 4 * 2.0 ** -53


@pytest.mark.parametrize("hyper", HYPERS, ids=IDS)
def test_adamw_step_is_torch_adamw_in_float64(hyper):
    """6 steps of one torch optimizer from zero moments against adamw_step, twice.
    Step by step: step t of the reference starts from the state torch reached
    after step t - 1 (the way the GPU tests resynchronise), and p', m', v' agree
    within 4 * 2^-53 relative per element.  Chained: the reference runs on its
    own from the start, never resynchronised; its p, the optimizer's result,
    stays within the same 4 * 2^-53 of torch's at every step.  Its m and v are
    held to t * 4 * 2^-53 at step t, not to the single limit: torch's lerp and
    addcmul and the definition's b m + (1 - b) x are different roundings of one
    formula, up to the per-step limit apart (asserted above), and with same-signed
    terms b m_(t-1) <= m_t, so the relative distance r_t <= r_(t-1) + that limit.
    m does reach 4.6 * 2^-53 after six steps here.
    Inputs: every element keeps its gradient's sign, so m never cancels, and |p|
    starts in [4, 8), far enough from zero for the largest lr here (0.6 in six
    steps); a relative limit means nothing where the value cancels."""
    rng = np.random.default_rng(1)
    n = 1000
    p = rng.choice([-1.0, 1.0], n) * rng.uniform(4.0, 8.0, n)
    sign = rng.choice([-1.0, 1.0], n)
    m, v = np.zeros(n), np.zeros(n)
    free = p.copy(), m.copy(), v.copy()
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"],
                            weight_decay=hyper["weight_decay"], foreach=False)
    worst, chained = 0.0, np.zeros(3)
    for t in range(1, 7):
        g = sign * rng.uniform(0.25, 4.0, n) * 2.0 ** rng.integers(-6, 3)
        mine = R.adamw_step(p, m, v, g, *ref_args(hyper), t)[:3]
        free = R.adamw_step(*free, g, *ref_args(hyper), t)[:3]
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[tp]
        p, m, v = (x.copy() for x in (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()))
        assert int(st["step"]) == t
        for name, a, b in zip("pmv", mine, (p, m, v)):
            e = rel(a, b)
            worst = max(worst, e)
            assert e <= LIMIT, (t, name, e)
        chained = np.array([rel(a, b) for a, b in zip(free, (p, m, v))])
        assert chained[0] <= LIMIT, (t, "chained p", chained[0])
        assert chained[1] <= t * LIMIT and chained[2] <= t * LIMIT, (t, "chained m, v", chained)
    print(f"worst relative difference from torch float64: {worst / 2.0 ** -53:.2f} * 2^-53 per step; chained, after "
          f"6 steps, p {chained[0] / 2.0 ** -53:.2f}, m {chained[1] / 2.0 ** -53:.2f}, v {chained[2] / 2.0 ** -53:.2f}")
    assert np.abs(p).min() > 2.0 and np.abs(m).min() > 0 and np.abs(v).min() > 0


def test_clip_coef_is_what_clip_grad_norm_applies():
    """clip_grad_norm_ (float64, its fixed eps 1e-6) scales every gradient by one
    coefficient; an element 1.0 in each tensor gives it back exactly.  Each
    tensor's norm is an integer (3-4-5 and the like) times a power of two, so
    torch's norm of the tensors' norms and the reference's square root of the sum
    of squares start from the same exact number.  Limit: 2 ulp of double."""
    base = [[3.0, 4.0], [5.0, 12.0], [8.0, 15.0], [1.0, 2.0, 2.0], [1.0]]
    seen = set()
    for e, max_norm in ((0, 3.0), (-3, 3.0), (-4, 3.0), (5, 0.1), (0, 1e9), (-20, 1e-3)):
        gs = [np.array(b) * 2.0 ** e for b in base]
        ts = [torch.zeros(x.size, dtype=torch.float64, requires_grad=True) for x in gs]
        for t, x in zip(ts, gs):
            t.grad = torch.from_numpy(x.copy())
        total = torch.nn.utils.clip_grad_norm_(ts, max_norm, foreach=False)
        sumsq = sum(float(np.sum(x * x)) for x in gs)        # exact: small integers times 4^e
        assert float(total) == np.sqrt(sumsq)
        want = R.clip_coef(sumsq, max_norm, 1e-6)
        for t, x in zip(ts, gs):
            got = t.grad.numpy() / x
            assert np.all(np.abs(got - want) <= 2 * np.spacing(want)), (e, max_norm, got, want)
        seen.add(bool(want < 1.0))
        assert (want == 1.0) == (max_norm >= np.sqrt(sumsq) + 1e-6)
    assert seen == {True, False}
    # the definition's edges
    assert R.clip_coef(0.0, 3.0, 0.0) == 1.0 and R.clip_coef(36.0, 3.0, 0.0) == 0.5
    assert R.clip_coef(9.0, 3.0, 0.0) == 1.0 and R.clip_coef(100.0, 3.0, 0.0) == np.float64(3.0) / np.float64(10.0)


# ---- the float32 statement inside the bounds -------------------------------------------

GCOEF, GRAD_MUL = 0.37, 2.0 ** -10


def state(n, seed, gdtype):
    """float32 p, m, v and a stored gradient with |g| in [2^-8, 2^15): with
    gcoef * grad_mul = 0.37 * 2^-10, |g_eff| in [2^-20, 2^6]; a tenth of m and of
    v exactly zero (a fresh state), the rest spread over decades"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    v = (10.0 ** rng.uniform(-12, 0, n)).astype(np.float32)
    m[rng.random(n) < 0.1] = 0.0
    v[rng.random(n) < 0.1] = 0.0
    g = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-8, 15, n)).astype(np.float32)
    stored = g if gdtype == "float" else H.from_f32(g, gdtype)
    return p, m, v, stored


def g_eff_of(stored, gdtype, c, grad_mul):
    """the effective gradient in float64: widen(g) * c * grad_mul"""
    return A.widen(stored, gdtype).astype(np.float64) * (np.float64(c) * np.float64(grad_mul))


def test_bound_constants_respect_the_ceilings():
    assert R.KM <= 6 and R.KV <= 9 and R.KP <= 4 and R.KQ <= 24 and R.U == 2.0 ** -24
    assert 1.0 < R.SLACK < 1.0 + 1e-5


@pytest.mark.parametrize("gdtype", TYPES)
@pytest.mark.parametrize("hyper", HYPERS, ids=IDS)
def test_sim_with_the_library_constants_stays_inside_the_bounds(hyper, gdtype):
    """adamw_sim.step with bine_adamw_consts' constants against adamw_step, one
    step from the same float32 state at steps 1, 2, 10, 1000 and 10^6"""
    gm = A.gm_of(GCOEF, GRAD_MUL)
    worst = np.zeros(3)
    for t in STEPS:
        p, m, v, g = state(N, 100 + t % 97, gdtype)
        ge = g_eff_of(g, gdtype, GCOEF, GRAD_MUL)
        assert 2.0 ** -20 <= np.abs(ge).min() and np.abs(ge).max() <= 2.0 ** 6
        ref = R.adamw_step(p, m, v, ge, *ref_args(hyper), t)
        assert ref[2].min() >= 2.0 ** -100                      # v' normal in float32, far from the edge
        got = A.step(p, m, v, g, gdtype, pico_amd.adamw_consts(step=t, **hyper), gm)
        r = np.array(R.ratios(got, ref))
        print(f"step {t}: |dp|, |dm|, |dv| at {r[0]:.3f}, {r[1]:.3f}, {r[2]:.3f} of their bounds")
        assert (r <= 1.0).all(), (t, r)
        worst = np.maximum(worst, r)
    # the bounds are not idle: the float32 statement uses a fair part of each
    assert (worst >= 0.1).all(), worst


def mutants(hyper, t):
    """float64 AdamW with one classic error each: what the bounds must reject"""
    lr, b1, b2, eps, wd = ref_args(hyper)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t

    def moments(m, v, g):
        return b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g

    def eps_inside(p, m, v, g):
        m1, v1 = moments(m, v, g)
        return p * (1 - lr * wd) - (lr / bc1) * m1 / ((np.sqrt(v1) + eps) / np.sqrt(bc2)), m1, v1

    def step_off_by_one(p, m, v, g):
        return R.adamw_step(p, m, v, g, lr, b1, b2, eps, wd, t + 1)[:3]

    def coupled_decay(p, m, v, g):
        return R.adamw_step(p, m, v, g + wd * p, lr, b1, b2, eps, 0.0, t)[:3]

    def no_bias_correction(p, m, v, g):
        m1, v1 = moments(m, v, g)
        return p * (1 - lr * wd) - lr * m1 / (np.sqrt(v1) + eps), m1, v1

    return [eps_inside, step_off_by_one, coupled_decay, no_bias_correction]


def test_bounds_reject_the_classic_errors():
    """each wrong formula, in exact float64, misses a bound by a factor above 100 on
    the inputs of the test above (hyper-parameters where the error exists at all:
    weight decay and eps not zero, a small step number)"""
    hyper, t = HYPERS[2], 2
    p, m, v, g = state(N, 7, "float")
    ge = g_eff_of(g, "float", GCOEF, GRAD_MUL)
    ref = R.adamw_step(p, m, v, ge, *ref_args(hyper), t)
    assert max(R.ratios(ref[:3], ref)) == 0.0
    for f in mutants(hyper, t):
        r = R.ratios(f(*(x.astype(np.float64) for x in (p, m, v)), ge), ref)
        print(f"{f.__name__}: {max(r):.3g} times a bound")
        assert max(r) > 100.0, (f.__name__, r)


def test_clip_coef_that_clamps_the_wrong_way_is_rejected():
    """max(1, r) in place of min(1, r): off by far more than the 4 ulp the GPU tests allow"""
    for sumsq in (1.0, 100.0):
        r = 3.0 / (np.sqrt(sumsq) + 1e-6)
        assert abs(max(1.0, r) - R.clip_coef(sumsq, 3.0, 1e-6)) > 0.5
