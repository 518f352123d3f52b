"""The numpy statement of the step-state update (include/bine_amd.h, "dynamic
loss scaling"): bine_step_update / bine_step_update_host, one float64
operation per line, and bine_step_state_init (test infrastructure).  numpy's
float64 +, -, *, / and sqrt are the IEEE operations, np.float32(x) of a float64
rounds once to nearest even, and numpy contracts nothing.  The state is the 96
bytes of the library's block: update() and init() return it as uint8.
"""
import numpy as np

BYTES = 96
FIELDS = ("scale", "good", "step", "pw1", "pw2", "skip", "gm", "skipped")
DBL_MAX = np.finfo(np.float64).max

# the hyper-parameters of bine_step_hyper, in its order, with the Python API's defaults
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=float("inf"), clip_eps=1e-6,
             growth_factor=2.0, backoff_factor=0.5, min_scale=1.0, max_scale=2.0 ** 24, growth_interval=2000)


def pack(d, c):
    return np.concatenate([np.asarray(d, dtype=np.float64).view(np.uint8), np.asarray(c, dtype=np.float32).view(np.uint8)])


def unpack(state):
    raw = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    assert raw.size == BYTES
    return raw[:64].copy().view(np.float64), raw[64:].copy().view(np.float32)


def init(scale, step, beta1, beta2):
    b1, b2 = np.float64(beta1), np.float64(beta2)
    pw1, pw2 = np.float64(1.0), np.float64(1.0)
    for _ in range(int(step)):
        pw1 = pw1 * b1
        pw2 = pw2 * b2
    return pack([scale, 0.0, float(step), pw1, pw2, 0.0, 0.0, 0.0], np.zeros(8))


def update(state, n2, **hyper):
    """the state after one update with the global squared norm n2"""
    h = {k: np.float64(v) for k, v in dict(HYPER, **hyper).items()}
    d, c = unpack(state)
    scale, good, step, pw1, pw2, skip, gm, skipped = d
    n2 = np.float64(n2)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        if not n2 <= DBL_MAX:
            skip = one
            gm = np.float64(0.0)
            skipped = skipped + one
            good = np.float64(0.0)
            scale = scale * h["backoff_factor"]
            scale = scale if scale > h["min_scale"] else h["min_scale"]
        else:
            inv = one / scale
            nrm = np.sqrt(n2)
            nrm = nrm * inv
            r = nrm + h["clip_eps"]
            r = h["max_norm"] / r
            cc = r if r < one else one
            gm = cc * inv
            step = step + one
            pw1 = pw1 * h["beta1"]
            pw2 = pw2 * h["beta2"]
            t = h["lr"] * h["weight_decay"]
            c[0] = np.float32(one - t)
            c[1] = np.float32(h["beta1"])
            c[2] = np.float32(one - h["beta1"])
            c[3] = np.float32(h["beta2"])
            c[4] = np.float32(one - h["beta2"])
            t = one - pw2
            t = np.sqrt(t)
            c[5] = np.float32(one / t)
            c[6] = np.float32(h["eps"])
            t = one - pw1
            c[7] = np.float32(h["lr"] / t)
            skip = np.float64(0.0)
            good = good + one
            if good >= h["growth_interval"]:
                scale = scale * h["growth_factor"]
                scale = scale if scale < h["max_scale"] else h["max_scale"]
                good = np.float64(0.0)
    return pack([scale, good, step, pw1, pw2, skip, gm, skipped], c)


def norms(seed, n=240, bad=0.12):
    """n global squared norms: finite ones over fifteen decades, with +inf, NaN
    and 0.0 among them"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        u = rng.random()
        if u < bad / 2:
            out.append(float("inf"))
        elif u < bad:
            out.append(float("nan"))
        elif u < bad + 0.04:
            out.append(0.0)
        else:
            out.append(float(10.0 ** rng.uniform(-3, 12)))
    return out


def cases():
    """(name, (scale, step), hyper, norms): the update sequences of the CPU and the
    GPU tests, 200 updates or more each"""
    inf, nan = float("inf"), float("nan")
    out = [("defaults, max_norm = inf", (65536.0, 0), {}, norms(1)),
           ("clipping", (1024.0, 0), dict(max_norm=1.0, growth_interval=7, lr=3e-4, beta1=0.95, beta2=0.98,
                                          eps=1e-6, weight_decay=0.0), norms(2)),
           ("beta1 = 0", (256.0, 0), dict(beta1=0.0, beta2=0.5, lr=0.1, eps=1e-3, weight_decay=0.3,
                                          growth_interval=3, max_norm=10.0, clip_eps=0.0), norms(3)),
           ("resumed at step 1000", (2.0 ** 20, 1000), dict(growth_interval=11, growth_factor=1.5,
                                                            backoff_factor=0.75, max_norm=0.5), norms(4)),
           # growth exactly at growth_interval = 5 and not one before it: 4 good, an overflow, 5 good, ...
           ("growth at the interval", (8.0, 0), dict(growth_interval=5),
            ([3.0] * 4 + [inf] + [3.0] * 5 + [nan] + [0.0] * 4 + [inf]) * 13),
           # the clamps: backing off onto min_scale, growing onto max_scale, and a max_scale the product overshoots
           ("min_scale", (4.0, 0), dict(min_scale=0.75), [inf, nan] * 100 + [2.0] * 5),
           ("max_scale", (2.0 ** 22, 0), dict(growth_interval=1, growth_factor=3.0, max_scale=2.0 ** 24),
            [1.0] * 100 + [inf] + [1.0] * 100)]
    return out


def fields(state):
    d, c = unpack(state)
    out = dict(zip(FIELDS, (float(x) for x in d)))
    out["consts"] = c
    return out
