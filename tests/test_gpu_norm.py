"""Global norm and clipping on the GPU: bine_sumsq_segments (k_sumsq_segs /
k_sumsq_fold / k_sumsq_total) against exact host sums, bine_clip_segments
(k_scale_segs) against numpy's float64 coefficient and the existing bine_scale,
and bine_norm_multi / bine_clip_multi over loopback ranks against the existing
loopback_allreduce on the vectors bine_sumsq_segments produced.  (Real processes
and graph mode: tools/norm_check.py, tests/test_gpu_norm_rccl.py.)"""
import math
from fractions import Fraction

import numpy as np
import pytest

import h16_util as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402

S = _lib.COPY_SEGS_PER_LAUNCH
ESZ = {"float": 4, "double": 8, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
GUARD = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def counts_of(dtype):
    """0, 1, one vector -1 / +0 / +1, one 32 KiB tile -1 / +0 / +1, 3 tiles + 21 elements"""
    vec, tile = 16 // ESZ[dtype], (32 << 10) // ESZ[dtype]
    return [0, 1, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1, 3 * tile + 21]


def encode(vals, dtype):
    """float64 values -> the type's storage (rounded to nearest even)"""
    if dtype == "double":
        return np.ascontiguousarray(vals, dtype=np.float64)
    if dtype == "float":
        return np.asarray(vals, dtype=np.float64).astype(np.float32)
    return H.from_f32(np.asarray(vals, dtype=np.float64).astype(np.float32), dtype)


def decode(stored, dtype):
    """the stored elements' values, exactly, as float64"""
    if dtype in H.TYPES:
        return H.to_f32(stored, dtype).astype(np.float64)
    return stored.astype(np.float64)


class Bucket:
    """tensors (count, phase in elements, null) in one arena of guard bytes, each
    with 16 guard bytes or more on either side; null: an empty tensor passed as
    NULL"""

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

    def values(self, k):
        return decode(self.data[k], self.dtype)

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


def mixed_specs(dtype, seed):
    """every count twice at random element-aligned phases, empties (some NULL) in between"""
    rng = np.random.default_rng(seed)
    per = 16 // ESZ[dtype]
    specs = []
    for rep in range(2):
        for c in counts_of(dtype):
            specs.append((c, int(rng.integers(0, per)), c == 0 and rep == 1))
        specs.append((0, 0, True))
    return specs


def many_specs(dtype, seed):
    """2 * 128 + 37 non-empty tensors, empties in between: three launches"""
    rng = np.random.default_rng(seed)
    per = 16 // ESZ[dtype]
    specs = []
    for k in range(2 * S + 37):
        specs.append((int(rng.choice([1, per - 1, per, per + 1, 100, 1025])), int(rng.integers(0, per)), False))
        if k % 5 == 0:
            specs.append((0, 0, k % 10 == 0))
    return specs


def bucket(dtype, specs, seed, kind):
    rng = np.random.default_rng(seed)
    data = []
    for c, _, _ in specs:
        if kind == "int":
            v = rng.integers(-8, 9, size=c).astype(np.float64)
        elif kind == "normal26":    # at most 26-bit significands: exact squares in binary64
            v = rng.standard_normal(c).astype(np.float32).astype(np.float64)
        else:
            v = rng.standard_normal(c)
        data.append(encode(v, dtype))
    return Bucket(dtype, specs, data)


class Guarded:
    """n float64 on the device between two guard doubles on either side"""
    PAT = 0x7FF8DEADBEEF0001

    def __init__(self, n, fill=None):
        self.n = n
        h = np.full(n + 4, self.PAT, dtype=np.uint64)
        if fill is not None:
            h[2:2 + n] = fill
        self.t = torch.from_numpy(h.view(np.int64).copy()).to("cuda:0")

    def ptr(self):
        return self.t.data_ptr() + 16

    def read(self):
        h = self.t.cpu().numpy().view(np.uint64)
        assert (h[:2] == self.PAT).all() and (h[2 + self.n:] == self.PAT).all(), "guard doubles changed"
        return h[2:2 + self.n].copy()


def run_sumsq(b, scratch_fill=None):
    """bine_sumsq_segments with an exactly sized scratch; returns out's bits"""
    n = len(b.counts)
    need = pico_amd.plan_sumsq([p or 0 for p in b.ptrs()], b.counts, b.dtype)
    out, scratch = Guarded(n + 1), Guarded(need, scratch_fill)
    pico_amd.sumsq_segments(b.ptrs(), b.dtype, counts=b.counts, out=out.ptr(), scratch=scratch.ptr(),
                            scratch_doubles=need)
    torch.cuda.synchronize()
    scratch.read()
    return out.read()


@pytest.mark.parametrize("dtype", TYPES)
def test_sumsq_exact_on_small_integers(dev, dtype):
    """integers in [-8, 8] are exact in every type and every partial sum is an
    integer below 2^53: any order gives the same bits as the host"""
    for specs in (mixed_specs(dtype, 1), many_specs(dtype, 2)):
        b = bucket(dtype, specs, 3, "int")
        got = run_sumsq(b).view(np.float64)
        want = [float(np.sum(b.values(k) ** 2)) for k in range(len(specs))]
        want.append(float(sum(want)))
        assert got.tobytes() == np.array(want, dtype=np.float64).tobytes()
        assert not np.signbit(got).any()          # empty tensors give +0.0
        assert b.unchanged(), "sumsq wrote to its input or around it"


@pytest.mark.parametrize("dtype", TYPES)
def test_sumsq_accuracy_and_determinism(dev, dtype):
    """random normal inputs: |out[k] - exact| <= counts[k] * 2^-52 * exact, exact =
    fsum of the exact squares; the same call with scratch full of NaN patterns
    gives the same bits"""
    b = bucket(dtype, mixed_specs(dtype, 4), 5, "normal26" if dtype == "double" else "normal")
    bits = run_sumsq(b)
    got = bits.view(np.float64)
    total = 0.0
    for k, c in enumerate(b.counts):
        v = b.values(k)
        exact = math.fsum((v * v).tolist())   # the squares are exact: at most 26-bit significands
        err, bound = abs(got[k] - exact), c * 2.0 ** -52 * exact
        print(f"{dtype} count {c}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (dtype, k, c, got[k], exact)
        assert c == 0 or bound < 1e-10 * exact
        total += got[k]
    assert got[-1] == total                    # out[n]: out[0] + ... + out[n - 1], in that order
    again = run_sumsq(b, scratch_fill=0xFFFFFFFFFFFFFFFF)
    assert again.tobytes() == bits.tobytes()
    assert b.unchanged()


def test_sumsq_double_full_significands(dev):
    specs = [(4097, 1, False), (21, 0, False)]
    b = bucket("double", specs, 6, "normal")
    got = run_sumsq(b).view(np.float64)
    for k, (c, _, _) in enumerate(specs):
        exact = sum(Fraction(float(x)) ** 2 for x in b.values(k))
        err, bound = abs(Fraction(float(got[k])) - exact), c * Fraction(1, 2 ** 52) * exact
        print(f"double count {c}: error {float(err):.3e}, bound {float(bound):.3e}")
        assert err <= bound


@pytest.mark.parametrize("dtype", TYPES)
def test_sumsq_ieee_cases(dev, dtype):
    specs = [(1025, 1, False), (0, 0, True), (40, 0, False), (3 * (32 << 10) // ESZ[dtype] + 5, 1, False)]
    b = bucket(dtype, specs, 7, "int")
    clean = run_sumsq(b).view(np.float64)
    for k, pos, val in ((0, 1024, np.inf), (3, specs[3][0] // 2, -np.inf), (2, 0, np.nan),
                        (3, specs[3][0] - 1, np.nan)):
        data = [x.copy() for x in b.data]
        data[k][pos] = encode([val], dtype)[0]
        got = run_sumsq(Bucket(dtype, specs, data)).view(np.float64)
        for j in range(len(specs)):
            if j != k:
                assert got[j] == clean[j], (dtype, k, j)       # that tensor and the total only
        if np.isnan(val):
            assert np.isnan(got[k]) and np.isnan(got[-1])
        else:
            assert got[k] == np.inf and got[-1] == np.inf
    if dtype in H.TYPES:     # subnormals are counted, exactly: patterns 1 .. 64 of the 16-bit format
        sub = np.arange(1, 65, dtype=np.uint16)
        got = run_sumsq(Bucket(dtype, [(64, 1, False)], [sub])).view(np.float64)
        want = math.fsum((decode(sub, dtype) ** 2).tolist())
        assert want > 0 and got[0] == want and got[1] == want


def np_coef(norm2, max_norm, eps):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float64(max_norm) / (np.sqrt(np.float64(norm2)) + np.float64(eps))
    return r if r < 1.0 else np.float64(1.0)


def dev_doubles(vals):
    return torch.from_numpy(np.array(vals, dtype=np.float64)).to("cuda:0")


def scaled_reference(b, c):
    """per tensor: the existing bine_scale with the coefficient, out of place"""
    want = []
    for k, cnt in enumerate(b.counts):
        src, dst = TG.to_dev(b.data[k], pad=16), torch.zeros(cnt * b.esz + 16, dtype=torch.uint8, device="cuda:0")
        if cnt:
            pico_amd.scale(src, dst, cnt, b.dtype, scale=float(c))
        torch.cuda.synchronize()
        want.append(dst[:cnt * b.esz].cpu().numpy())
    return want


MAXN = 3.0
ABOVE, BELOW = float(np.nextafter(9.0, 10.0)), float(np.nextafter(9.0, 8.0))
CLIP_CASES = [(100.0, 1e-6), (0.0, 0.0), (float("nan"), 1e-6), (ABOVE, 0.0), (BELOW, 0.0), (1e300, 0.0)]


@pytest.mark.parametrize("dtype", TYPES)
def test_clip_segments(dev, dtype):
    specs = mixed_specs(dtype, 8)
    ref = {}
    for norm2, eps in CLIP_CASES:
        b = bucket(dtype, specs, 9, "normal")
        c = np_coef(norm2, MAXN, eps)
        nd, coef = dev_doubles([norm2]), Guarded(1)
        pico_amd.clip_segments(b.ptrs(), nd, MAXN, eps, dtype=dtype, counts=b.counts, coef_out=coef.ptr())
        torch.cuda.synchronize()
        got_c = coef.read().view(np.float64)[0]
        assert got_c.tobytes() == np.float64(c).tobytes(), (norm2, eps, got_c, c)
        parts, guards = b.read()
        assert guards, "bytes around a tensor changed"
        if c == 1.0:
            assert b.unchanged(), (norm2, eps)
            continue
        if float(c) not in ref:
            ref[float(c)] = scaled_reference(b, c)
        for k, (p, w) in enumerate(zip(parts, ref[float(c)])):
            assert p.tobytes() == w.tobytes(), (dtype, norm2, k, b.counts[k])
    assert np_coef(ABOVE, MAXN, 0.0) < 1.0 and np_coef(BELOW, MAXN, 0.0) == 1.0 and len(ref) == 3
    # more than one launch; coef_out may be NULL; nothing to scale still stores the coefficient
    b = bucket(dtype, many_specs(dtype, 10), 11, "normal")
    nd = dev_doubles([36.0])
    pico_amd.clip_segments(b.ptrs(), nd, MAXN, 0.0, dtype=dtype, counts=b.counts)
    torch.cuda.synchronize()
    parts, guards = b.read()
    assert guards
    for p, w in zip(parts, scaled_reference(b, 0.5)):
        assert p.tobytes() == w.tobytes()
    coef = Guarded(1)
    pico_amd.clip_segments([None, None], nd, MAXN, 0.0, dtype=dtype, counts=[0, 0], coef_out=coef.ptr())
    pico_amd.clip_segments([], nd, 1.5, 0.0, dtype=dtype, counts=[], coef_out=coef.ptr())
    torch.cuda.synchronize()
    assert coef.read().view(np.float64)[0] == 0.25


def round_once(y, dtype):
    """float64 -> the 16-bit type's bits, one rounding to nearest even (normal range)"""
    if dtype == "float16":
        return np.asarray(y, dtype=np.float64).astype(np.float16).view(np.uint16)
    m, e = np.frexp(np.asarray(y, dtype=np.float64))
    r = np.ldexp(np.round(m * 256.0), e - 8)          # 8 significant bits; numpy rounds halves to even
    assert (np.abs(r[r != 0]) > 1e-30).all()
    return H.from_f32(r.astype(np.float32), dtype)    # exact: r is a bfloat16 value


@pytest.mark.parametrize("dtype", TYPES)
def test_clip_segments_against_the_host(dev, dtype):
    """the clipped tensors against the product computed here, no kernel of the
    library involved: float and double bit for bit (x * (float)c, x * c); the
    16-bit types bit for bit the header's two roundings (binary32 product, then
    the type), hence the single rounding of the float64 product x * c wherever
    the two agree, and never more than one unit in the last place from it"""
    import optim_ref as R
    eps = 1e-6
    c = R.clip_coef(100.0, MAXN, eps)
    assert 0.29 < c < 0.3
    b = bucket(dtype, mixed_specs(dtype, 12), 13, "normal")
    nd, coef = dev_doubles([100.0]), Guarded(1)
    pico_amd.clip_segments(b.ptrs(), nd, MAXN, eps, dtype=dtype, counts=b.counts, coef_out=coef.ptr())
    torch.cuda.synchronize()
    assert coef.read().view(np.float64)[0] == c
    parts, guards = b.read()
    assert guards, "bytes around a tensor changed"
    cf = np.float64(np.float32(c))
    agree = total = 0
    for k, cnt in enumerate(b.counts):
        x = b.values(k)                                  # the stored values, exactly, as float64
        if dtype == "double":
            assert parts[k].tobytes() == (x * c).tobytes(), (k, cnt)
            continue
        prod32 = (x * cf).astype(np.float32)             # x and (float)c have 24 bits each: one rounding
        if dtype == "float":
            assert parts[k].tobytes() == prod32.tobytes(), (k, cnt)
            continue
        got = parts[k].view(np.uint16)
        two, one = H.from_f32(prod32, dtype), round_once(x * c, dtype)
        assert got.tobytes() == two.tobytes(), (k, cnt)
        same = two == one
        assert np.array_equal(got[same], one[same])
        # same sign, finite: the patterns are ordered like the magnitudes
        assert (np.abs(got.astype(np.int32) - one.astype(np.int32)) <= 1).all(), (k, cnt)
        agree, total = agree + int(same.sum()), total + cnt
    if dtype in H.TYPES:
        print(f"{dtype}: two roundings equal the single one on {agree} of {total} elements")
        assert 0.9 * total < agree


# ---- the collectives over loopback ranks ---------------------------------------------------

def rank_buckets(dtype, P, seed):
    """per rank: eight tensors whose counts differ from rank to rank (shards do)"""
    per, tile = 16 // ESZ[dtype], (32 << 10) // ESZ[dtype]
    base = [0, 1, per + 1, 1023, tile, tile + 1, 2 * tile + 21, 5]
    out = []
    for r in range(P):
        specs = [(c + (r * (k + 1) if c else 0), (k + r) % per, c == 0 and r % 2 == 1) for k, c in enumerate(base)]
        out.append(bucket(dtype, specs, seed + r, "normal"))
    return out


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_norm_multi_is_the_single_allreduce(dev, P):
    cs = TG.comms(P)
    compared = 0
    for dtype in ("float", "bfloat16"):
        bs = rank_buckets(dtype, P, 20 + P)
        n = len(bs[0].counts)
        V = [run_sumsq(b) for b in bs]
        for algo in ("recursivedoubling", "bine_lat"):
            single = [torch.from_numpy(v.view(np.int64).copy()).to("cuda:0") for v in V]
            torch.cuda.synchronize()
            _, est = pico_amd.loopback_allreduce(cs, algo, [pico_amd.IN_PLACE] * P, single, n + 1, "double", "sum")
            torch.cuda.synchronize()
            stats = [Guarded(n + 1) for _ in range(P)]
            _, st = pico_amd.loopback_norm_multi(cs, algo, [b.ptrs() for b in bs], dtype, [s.ptr() for s in stats],
                                                 counts=[b.counts for b in bs])
            torch.cuda.synchronize()
            assert st == est, (dtype, algo, st, est)      # what the single call refuses is returned as it returns it
            if any(est):
                continue
            for r in range(P):
                assert stats[r].read().tobytes() == single[r].cpu().numpy().tobytes(), (dtype, algo, r)
                assert bs[r].unchanged()
            compared += 1
            # against the host: the ranks' exact sums, within the kernel's bound summed over the ranks
            got = stats[0].read().view(np.float64)
            for k in range(n):
                exact = math.fsum(x for b in bs for x in (b.values(k) ** 2).tolist())
                assert abs(got[k] - exact) <= (sum(b.counts[k] for b in bs) + P) * 2.0 ** -52 * exact
    print(f"P={P}: {compared} calls compared")
    assert compared == 4                                  # both latency algorithms take every P here


@pytest.mark.parametrize("P", [1, 2, 4])
def test_clip_multi_is_norm_multi_then_clip_segments(dev, P):
    cs = TG.comms(P)
    for dtype, max_norm in (("float", 7.5), ("bfloat16", 1e9)):
        bs, ref = rank_buckets(dtype, P, 40 + P), rank_buckets(dtype, P, 40 + P)
        n = len(bs[0].counts)
        stats = [Guarded(n + 2) for _ in range(P)]
        _, st = pico_amd.loopback_clip_multi(cs, "bine_lat", [b.ptrs() for b in bs], dtype, max_norm, 1e-6,
                                             [s.ptr() for s in stats], counts=[b.counts for b in bs])
        torch.cuda.synchronize()
        assert st == [0] * P
        got = [s.read() for s in stats]
        norm = [Guarded(n + 1) for _ in range(P)]
        _, st = pico_amd.loopback_norm_multi(cs, "bine_lat", [b.ptrs() for b in ref], dtype, [s.ptr() for s in norm],
                                             counts=[b.counts for b in ref])
        torch.cuda.synchronize()
        assert st == [0] * P
        for r in range(P):
            assert got[r][:n + 1].tobytes() == norm[r].read().tobytes()
            assert got[r][n + 1] == got[0][n + 1]                 # the same coefficient bits on every rank
            nd, coef = dev_doubles(got[r][n:n + 1].view(np.float64)), Guarded(1)
            pico_amd.clip_segments(ref[r].ptrs(), nd, max_norm, 1e-6, dtype=dtype, counts=ref[r].counts,
                                   coef_out=coef.ptr())
            torch.cuda.synchronize()
            assert coef.read()[0] == got[r][n + 1]
            assert bs[r].t.cpu().numpy().tobytes() == ref[r].t.cpu().numpy().tobytes()
        c = got[0][n + 1:].view(np.float64)[0]
        assert (c < 1.0) == (dtype == "float"), c                 # one case clips, the other does not
        if c == 1.0:
            assert all(b.unchanged() for b in bs)
