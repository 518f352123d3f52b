"""AdamW with decoupled weight decay and global-norm clipping in float64, written
from the algorithms' definitions (Loshchilov & Hutter, "Decoupled Weight Decay
Regularization", algorithm 2; Pascanu et al. for the clipping), and the float32
forward-error bounds of one step of bine_adamw_segments against it (test
infrastructure, numpy only).  Nothing here comes from the library: no constant
of bine_adamw_consts, no line of tests/adamw_sim.py.  tests/test_optim_ref.py
pins adamw_step and clip_coef to torch.optim.AdamW / clip_grad_norm_ in float64
and shows that the float32 statement of the contract stays inside bounds().
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of binary32, round to nearest


def clip_coef(total_sumsq, max_norm, eps):
    """min(1, max_norm / (sqrt(total_sumsq) + eps)) in float64"""
    with np.errstate(divide="ignore"):
        r = np.float64(max_norm) / (np.sqrt(np.float64(total_sumsq)) + np.float64(eps))
    return np.float64(min(1.0, float(r)))


def adamw_step(p, m, v, g_eff, lr, beta1, beta2, eps, wd, t):
    """step t (1-based) from state (p, m, v) with the effective gradient g_eff (the
    stored gradient times the clip coefficient times 1 / loss scale), all float64:
        m' = b1 m + (1 - b1) g           v' = b2 v + (1 - b2) g^2
        p' = p (1 - lr wd) - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    Returns (p', m', v', ma, pa, ua), the last three the magnitudes bounds() needs:
    ma = b1 |m| + (1 - b1) |g|, pa = |p| (1 - lr wd), ua = (lr / (1 - b1^t)) ma / d."""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g_eff))
    lr, b1, b2, eps, wd = (float(x) for x in (lr, beta1, beta2, eps, wd))
    t = int(t)
    assert t >= 1
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * (g * g)
    d = np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps
    step_size = lr / (1.0 - b1 ** t)
    p1 = p * (1.0 - lr * wd) - step_size * (m1 / d)
    ma = b1 * np.abs(m) + (1.0 - b1) * np.abs(g)
    pa = np.abs(p) * (1.0 - lr * wd)
    ua = step_size * ma / d
    return p1, m1, v1, ma, pa, ua


# The bounds.  The float32 side (include/bine_amd.h, bine_adamw_segments) starts from
# the same float32 p, m, v, the same stored gradient and the same double
# hyper-parameters, and performs, every operation rounded once to nearest
# (relative error at most u each, written (1+u) below):
#
#   constants  dk, b1, 1 - b1, b2, 1 - b2, eps: the double value rounded once     1 each
#              rbc2 = 1 / sqrt(1 - b2^t), ss = lr / (1 - b1^t): one rounding and
#              one ulp (<= 2u) for the library's pow                              3 each
#   gm = (float)(c * grad_mul)            the double product rounded once         1
#   gs = g * gm                           gm, the product                         2
#
#   m' = (m * b1) + (gs * (1 - b1))
#        m * b1:  the constant, the product                                       2
#        gs * (1 - b1):  gs, the constant, the product                            4
#        the sum rounds both terms once more:  b1 |m| carries 3, (1 - b1) |g|
#        carries 5, and |sum of the errors| <= 5u (b1 |m| + (1 - b1) |g|)
#                                                              |dm| <= 5u ma
#   v' = (v * b2) + ((gs * gs) * (1 - b2))
#        v * b2:  2;   gs * gs:  2 + 2 + 1 = 5;   * (1 - b2):  5 + 1 + 1 = 7
#        the sum:  + 1; every term is non-negative, so relative to v' itself
#                                                              |dv| <= 8u v'
#   d  = (sqrt(v') * rbc2) + eps
#        sqrt halves v's 8 and rounds:  4 + 1 = 5;   * rbc2:  5 + 3 + 1 = 9
#        eps:  1;  both terms non-negative, the sum rounds once:  <= 9 + 1 = 10
#   q  = ss * (m' / d)
#        m' / d:  |dm| / d <= 5u ma / d,  d's 10 on |m'| / d <= ma / d,  the
#        quotient's rounding 1:  16u ma / d;   ss * ...:  16 + 3 + 1 = 20
#                                                              |dq| <= 20u ua
#   p' = (p * dk) - q
#        p * dk:  2u pa;  the difference rounds once, u |p dk - q| <= u (pa + ua)
#                                                       |dp| <= u (3 pa + 21 ua)
#
# 5, 8 and (3, 21): below the ceilings 6, 9 and (4, 24).  The counts are first
# order in u.  The second-order terms of at most 21 factors (1+u)^(+-1), the
# square root's and the quotient's included, are below 21^2 u^2, and the float64
# side's own roundings (a dozen of 2^-53, and pow's error in 1 - b^t at small t)
# are below 2^-40 relative: SLACK = 1 / (1 - 64 u) = 1 + 3.8e-6 covers both.
# Assumed: the normal range -- |g_eff| in [2^-20, 2^6] and v' normal; then the
# only operation that can underflow is m * b1 (absolute error 2^-150, far below
# SLACK's share of 5u ma >= 5u (1 - b1) 2^-20).
KM, KV, KP, KQ = 5.0, 8.0, 3.0, 21.0
SLACK = 1.0 / (1.0 - 64.0 * U)


def bounds(v1, ma, pa, ua):
    """(bm, bv, bp): per element |m'_32 - m'|, |v'_32 - v'|, |p'_32 - p'| of one float32
    step against adamw_step's float64 v' and magnitudes ma, pa, ua"""
    v1, ma, pa, ua = (np.asarray(x, dtype=np.float64) for x in (v1, ma, pa, ua))
    return KM * U * SLACK * ma, KV * U * SLACK * v1, U * SLACK * (KP * pa + KQ * ua)


def ratios(got, ref):
    """the worst |got - ref| / bound of (p, m, v): got = the float32 (p', m', v'),
    ref = adamw_step's tuple; an empty tensor gives zeros"""
    p1, m1, v1, ma, pa, ua = ref
    bm, bv, bp = bounds(v1, ma, pa, ua)
    out = []
    for x, r, b in ((got[0], p1, bp), (got[1], m1, bm), (got[2], v1, bv)):
        x = np.asarray(x, dtype=np.float64)
        assert x.shape == r.shape and np.isfinite(x).all() and (b > 0).all()
        out.append(float(np.max(np.abs(x - r) / b)) if x.size else 0.0)
    return tuple(out)
