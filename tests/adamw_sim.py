"""The numpy float32 statement of bine_adamw_segments (include/bine_amd.h), one
numpy operation per line: what k_adamw_segs must reproduce bit for bit (test
infrastructure).  The constants come from bine_adamw_consts, the 16-bit types
widen and narrow through h16_util.  numpy's float32 +, -, *, / and sqrt are the
IEEE operations (nearest even, subnormals kept), and numpy contracts nothing.
"""
import numpy as np

import h16_util as H
import pico_amd

GM_ONE = np.float32(1.0)


def gm_of(gcoef=None, grad_mul=1.0):
    """(float)(c * grad_mul): the product in float64, one rounding"""
    c = np.float64(1.0 if gcoef is None else gcoef)
    with np.errstate(all="ignore"):
        return np.float32(c * np.float64(grad_mul))


def widen(g, gdtype):
    """stored gradient (float32, or uint16 patterns) -> float32, exactly"""
    return np.ascontiguousarray(g, dtype=np.float32) if gdtype == "float" else H.to_f32(g, gdtype)


def narrow(p, odtype):
    """float32 -> the stored type, nearest even (float: p itself)"""
    return np.ascontiguousarray(p, dtype=np.float32) if odtype == "float" else H.from_f32(p, odtype)


def step(p, m, v, g, gdtype, consts, gm=GM_ONE):
    """(p', m', v') as float32 arrays; p, m, v float32, g as stored"""
    dk, b1, omb1, b2, omb2, rbc2, eps, ss = (np.float32(c) for c in consts)
    p, m, v = (np.ascontiguousarray(x, dtype=np.float32) for x in (p, m, v))
    gm = np.float32(gm)
    with np.errstate(all="ignore"):
        gs = widen(g, gdtype) * gm
        p1 = p * dk
        t = m * b1
        u = gs * omb1
        m1 = t + u
        t = v * b2
        u = gs * gs
        u = u * omb2
        v1 = t + u
        d = np.sqrt(v1)
        d = d * rbc2
        d = d + eps
        q = m1 / d
        q = ss * q
        p2 = p1 - q
    assert p2.dtype == m1.dtype == v1.dtype == np.float32
    return p2, m1, v1


def adamw(p, m, v, g, gdtype, lr, beta1, beta2, eps, weight_decay, step_no, gcoef=None, grad_mul=1.0):
    """the whole call on one tensor: constants through bine_adamw_consts"""
    consts = pico_amd.adamw_consts(lr, beta1, beta2, eps, weight_decay, step_no)
    return step(p, m, v, g, gdtype, consts, gm_of(gcoef, grad_mul))
