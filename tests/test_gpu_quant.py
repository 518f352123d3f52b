"""FP8 quantization on the GPU: bine_amax_segments, bine_fp8_scales,
bine_quant_segments and bine_dequant_segments against tests/fp8_sim.py, the
numpy statement of the header's contract, bit for bit on both bodies, and
bine_quant_multi over loopback ranks against the sim's five steps and against
the five public calls issued one by one.  (Real processes and graph mode:
tools/quant_check.py, tests/test_gpu_quant_rccl.py.)"""
import numpy as np
import pytest

import fp8_sim as F
import h16_util as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402

S = _lib.COPY_SEGS_PER_LAUNCH
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
GUARD = 0xA5


def counts_of(dtype):
    """0, 1, one 16-B vector -1 / +0 / +1, one 32 KiB tile -1 / +0 / +1, 3 tiles + 21"""
    v = 16 // ESZ[dtype]
    tile = 2048 * v
    return [0, 1, v - 1, v, v + 1, tile - 1, tile, tile + 1, 3 * tile + 21]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Bucket:
    """tensors (count, phase in BYTES, null) of `esz`-byte elements in one arena
    of guard bytes, each with 16 guard bytes or more on either side; null: an
    empty tensor passed as NULL; data None: the tensor starts as guard bytes"""

    def __init__(self, esz, specs, data=None):
        self.esz, self.specs = esz, specs
        self.off, o = [], 0
        for c, ph, _ in specs:
            self.off.append(o + 16 + ph)
            o = (o + 16 + ph + c * esz + 16 + 15) & ~15
        self.host = np.full(o + 16, GUARD, dtype=np.uint8)
        if data is not None:
            for (c, _, _), f, x in zip(specs, self.off, data):
                x = np.ascontiguousarray(x)
                assert x.size == c and x.itemsize == esz
                self.host[f:f + c * esz] = x.view(np.uint8)
        self.t = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0
        self.counts = [c for c, _, _ in specs]

    def ptrs(self):
        return [None if null else self.t.data_ptr() + f for (_, _, null), f in zip(self.specs, self.off)]

    def unchanged(self):
        return bool(np.array_equal(self.t.cpu().numpy(), self.host))

    def read(self, view=np.uint8):
        """(the tensors, whether every other byte is as it was)"""
        got = self.t.cpu().numpy()
        mask = np.zeros(got.size, dtype=bool)
        parts = []
        for c, f in zip(self.counts, self.off):
            mask[f:f + c * self.esz] = True
            parts.append(got[f:f + c * self.esz].copy().view(view))
        return parts, bool(np.array_equal(got[~mask], self.host[~mask]))


def words(n, fill=0x5A5A5A5A, dtype=torch.int32):
    """n 4-byte words on the device between two guard words of 4"""
    t = torch.full((n + 8,), fill, dtype=torch.int32, device="cuda:0").view(dtype)
    return t, t[4:4 + n]


def guards_ok(t, n, fill=0x5A5A5A5A):
    a = t.view(torch.int32).cpu().numpy()
    return bool((a[:4] == fill).all() and (a[4 + n:] == fill).all())


# ---- inputs --------------------------------------------------------------------------------

def random_wide(dtype, n, rng):
    """normal values over many binades, signs, a few zeros and subnormals"""
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    x[rng.integers(0, 9, n) == 0] = 0.0
    return x if dtype == "float" else H.from_f32(x, dtype)


def from_values(dtype, v):
    v = np.asarray(v, dtype=np.float32)
    return v if dtype == "float" else H.from_f32(v, dtype)


def mixed_specs(dtype, seed, dphases=(0, 1, 2, 3)):
    """every count at source phases 0 and 1 element off 16 B and every
    destination phase: (count, source phase in bytes, destination phase)"""
    esz = ESZ[dtype]
    return [(c, sp * esz, dp) for c in counts_of(dtype) for sp in (0, 1) for dp in dphases]


# ---- bine_amax_segments ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES)
def test_amax_segments_is_the_sim(dev, dtype):
    rng = np.random.default_rng(11)
    esz, v = ESZ[dtype], 16 // ESZ[dtype]
    specs = [(c, sp, False) for c, sp, _ in mixed_specs(dtype, 0, dphases=(0,))]
    data = [random_wide(dtype, c, rng) for c, _, _ in specs]
    big = 3 * 2048 * v + 21
    # a NaN in a head, a body and a tail position (source one element off: the head is v - 1 elements), an
    # infinity, all zeros, -0 alone, the largest finite value, one subnormal
    nan, ninf = from_values(dtype, [np.nan])[0], from_values(dtype, [-np.inf])[0]
    for pos in (0, v + 5, 2048 * v + 77, big - 1):
        x = random_wide(dtype, big, rng)
        x[pos] = nan
        specs.append((big, esz, False))
        data.append(x)
    x = random_wide(dtype, big, rng)
    x[4000] = ninf
    extra = [x, from_values(dtype, np.zeros(2 * v + 3)), from_values(dtype, [-0.0]),
             from_values(dtype, [1.0, -3.0e38 if dtype != "float16" else -65504.0, 2.0]),
             np.array([3], dtype=np.uint32).view(np.float32) if dtype == "float" else np.array([3], dtype=np.uint16)]
    for x in extra:
        specs.append((x.size, esz, False))
        data.append(x)
    specs += [(0, 0, True), (0, 0, False)]
    data += [data[0][:0], data[0][:0]]
    b = Bucket(esz, specs, data)
    n = len(specs)
    t, out = words(n)
    pico_amd.amax_segments(b.ptrs(), dtype=dtype, counts=b.counts, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    want = np.array([F.amax_bits(x, dtype) for x in data], dtype=np.uint32)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert b.unchanged() and guards_ok(t, n)
    assert (want[len(specs) - 11:len(specs) - 7] > 0x7F800000).all() and want[-7] == 0x7F800000
    assert want[-6] == 0 and want[-5] == 0 and want[-1] == 0


@pytest.mark.parametrize("dtype", TYPES)
def test_amax_workgroups_of_several_tiles(dev, dtype):
    """a workgroup takes BINE_AMAX_TILES_PER_WG = 4 consecutive tiles: tensors of
    G - 1, G, G + 1 and 2 G + 1 tiles and a few elements, the one largest
    magnitude planted in the first and the last element of every tile in turn"""
    G, v = 4, 16 // ESZ[dtype]
    tile = 2048 * v
    rng = np.random.default_rng(29)
    specs, data = [], []
    for tiles, extra, sp in ((G - 1, 0, 0), (G, 0, 0), (G, 1, ESZ[dtype]), (G + 1, 0, 0), (2 * G + 1, 5, ESZ[dtype])):
        c = tiles * tile + extra
        for t in range(tiles + (1 if extra else 0)):
            for pos in (t * tile, min((t + 1) * tile, c) - 1):
                x = from_values(dtype, np.clip(F.widen(random_wide(dtype, c, rng), dtype), -100.0, 100.0))
                x[pos] = from_values(dtype, [-30000.0])[0]
                specs.append((c, sp, False))
                data.append(x)
    b = Bucket(ESZ[dtype], specs, data)
    n = len(specs)
    t, out = words(n)
    pico_amd.amax_segments(b.ptrs(), dtype=dtype, counts=b.counts, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    want = int(np.float32(30000.0).view(np.uint32)) if dtype != "bfloat16" else F.amax_bits(data[0], dtype)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    assert got.tolist() == [F.amax_bits(x, dtype) for x in data]
    assert b.unchanged() and guards_ok(t, n)


@pytest.mark.parametrize("n", [1, S - 1, S, S + 1])
def test_amax_list_lengths(dev, n):
    rng = np.random.default_rng(n)
    dtype = TYPES[n % 3]
    specs = []
    for k in range(n):
        c = 0 if k % 5 == 3 else int(rng.integers(1, 70))
        specs.append((c, int(rng.integers(0, 8)) * ESZ[dtype], c == 0 and k % 2 == 0))
    data = [random_wide(dtype, c, rng) for c, _, _ in specs]
    b = Bucket(ESZ[dtype], specs, data)
    t, out = words(n)
    pico_amd.amax_segments(b.ptrs(), dtype=dtype, counts=b.counts, out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [F.amax_bits(x, dtype) for x in data]
    assert b.unchanged() and guards_ok(t, n)


# ---- bine_fp8_scales ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", F.FORMATS)
def test_fp8_scales_is_the_sim(dev, fmt):
    pats = F.boundary_patterns(fmt)
    for lo in range(0, len(pats), 1000):
        chunk = pats[lo:lo + 1000]
        n = len(chunk)
        amax = torch.from_numpy(np.array(chunk, dtype=np.uint32).view(np.int32)).to(dev)
        t, scales = words(2 * n, dtype=torch.float32)
        pico_amd.fp8_scales(amax, fmt, n, scales=scales)
        torch.cuda.synchronize()
        got = scales.cpu().numpy()
        want = [F.scale_rule(p, fmt) for p in chunk]
        assert got[:n].tobytes() == np.array([s for s, _ in want], dtype=np.float32).tobytes()
        assert got[n:].tobytes() == np.array([i for _, i in want], dtype=np.float32).tobytes()
        assert guards_ok(t, 2 * n)


# ---- bine_quant_segments -------------------------------------------------------------------------------

def run_quant(dtype, fmt, specs, data, scales):
    """specs: (count, source phase in bytes, destination phase); returns the bytes per tensor"""
    src = Bucket(ESZ[dtype], [(c, sp, c == 0 and sp == 0) for c, sp, _ in specs], data)
    dst = Bucket(1, [(c, dp, c == 0 and dp == 0) for c, _, dp in specs])
    sc = None if scales is None else torch.from_numpy(np.asarray(scales, dtype=np.float32)).to("cuda:0")
    pico_amd.quant_segments(src.ptrs(), dst.ptrs(), fmt, scales=sc, sdtype=dtype, counts=src.counts)
    torch.cuda.synchronize()
    got, guards = dst.read()
    assert guards, "bytes outside the destinations changed"
    assert src.unchanged()
    return got


def check_quant(dtype, fmt, specs, data, scales):
    got = run_quant(dtype, fmt, specs, data, scales)
    for k, x in enumerate(data):
        want = F.quant(x, dtype, fmt, 1.0 if scales is None else scales[k])
        bad = np.nonzero(got[k] != want)[0]
        assert bad.size == 0, (dtype, fmt, k, specs[k], bad[:4], x[bad[:4]], got[k][bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("dtype", H.TYPES)
def test_quant_all_16bit_patterns(dev, dtype, fmt):
    """every pattern of the source type, NaNs included, at scales 1, 2^-3 and 2^5,
    through the vector body and (destination off by 3) the element body"""
    x = F.all16(dtype)
    scales = [1.0, 2.0 ** -3, 2.0 ** 5, 1.0, 2.0 ** -3, 2.0 ** 5]
    specs = [(x.size, 0, 0), (x.size, 2, 1), (x.size, 0, 8), (x.size, 2, 4), (x.size, 0, 3), (x.size, 14, 7)]
    check_quant(dtype, fmt, specs, [x] * 6, scales)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_quant_float_midpoints(dev, fmt):
    """every rounding boundary of the format and the float32 values one ulp
    either side, the clamp, the infinities, NaNs of both signs"""
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    x = np.concatenate([F.midpoints(fmt), nans])
    specs = [(x.size, 0, 0), (x.size, 4, 3), (x.size, 12, 1), (x.size, 8, 2)]
    check_quant("float", fmt, specs, [x] * 4, None)
    # the same values reached through a scale: x / 8 times 8
    with np.errstate(invalid="ignore"):
        eighth = x * np.float32(0.125)
    check_quant("float", fmt, specs[:2], [eighth] * 2, [8.0, 8.0])


@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("dtype", TYPES)
def test_quant_segments_bodies_heads_and_tails(dev, dtype, fmt):
    """every count at both source phases and all four destination phases, random
    data at the scale the rule gives: amax_segments, fp8_scales, quant_segments"""
    rng = np.random.default_rng(23)
    specs = mixed_specs(dtype, 0)
    data = [random_wide(dtype, c, rng) for c, _, _ in specs]
    n = len(specs)
    src = Bucket(ESZ[dtype], [(c, sp, False) for c, sp, _ in specs], data)
    dst = Bucket(1, [(c, dp, False) for c, _, dp in specs])
    amax = pico_amd.amax_segments(src.ptrs(), dtype=dtype, counts=src.counts)
    scales = pico_amd.fp8_scales(amax, fmt, n=n)
    pico_amd.quant_segments(src.ptrs(), dst.ptrs(), fmt, scales=scales, sdtype=dtype, counts=src.counts)
    torch.cuda.synchronize()
    got, guards = dst.read()
    assert guards and src.unchanged()
    sc = scales.cpu().numpy()
    plan = pico_amd.plan_quant([p or 0 for p in src.ptrs()], [p or 0 for p in dst.ptrs()], src.counts, dtype)
    assert {r[4] for r in plan} == {0, 1}, "both bodies run"
    for k, x in enumerate(data):
        s, i = F.scale_rule(F.amax_bits(x, dtype), fmt)
        assert sc[k] == s and sc[n + k] == i
        assert np.array_equal(got[k], F.quant(x, dtype, fmt, s)), (k, specs[k])
        if x.size and np.abs(F.widen(x, dtype)).max() > 0:
            top = (got[k] & 0x7F).max()              # the scale fills the format: FMAX / 2 < amax * scale <= FMAX
            assert (0x76 if fmt == "e4m3" else 0x77) <= top <= (0x7E if fmt == "e4m3" else 0x7B), (k, top)


@pytest.mark.parametrize("n", [1, S - 1, S, S + 1])
def test_quant_list_lengths(dev, n):
    rng = np.random.default_rng(100 + n)
    dtype, fmt = TYPES[n % 3], F.FORMATS[n % 2]
    specs = []
    for k in range(n):
        c = 0 if k % 5 == 3 else int(rng.integers(1, 70))
        specs.append((c, (0 if c == 0 and k % 2 == 0 else int(rng.integers(0, 8)) * ESZ[dtype]),
                      0 if c == 0 and k % 2 == 0 else int(rng.integers(0, 16))))
    data = [random_wide(dtype, c, rng) for c, _, _ in specs]
    scales = np.exp2(rng.integers(-4, 5, n)).astype(np.float32)
    check_quant(dtype, fmt, specs, data, scales)


# ---- bine_dequant_segments ------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("dtype", TYPES)
def test_dequant_all_bytes(dev, dtype, fmt):
    """all 256 bytes, repeated past one tile, at inverse scales 1, 2^-3, 2^5 and
    two that round in the 16-bit types; both bodies, heads and tails"""
    esz, v = ESZ[dtype], 16 // ESZ[dtype]
    reps = (2048 * v) // 256 + 2
    b = np.tile(np.arange(256, dtype=np.uint8), reps)[:2048 * v + 256 + 5]
    invs = [1.0, 2.0 ** -3, 2.0 ** 5, 1.0 / 3.0, 2.0 ** -120, 1.0]
    specs = [(b.size, 0, 0), (b.size, 1, esz), (b.size, 3, 0), (b.size, 2, 3 * esz), (b.size, 0, esz), (256, 5, 0)]
    data = [b[:c] for c, _, _ in specs]
    src = Bucket(1, [(c, sp, False) for c, sp, _ in specs], data)
    dst = Bucket(esz, [(c, dp, False) for c, _, dp in specs])
    inv = torch.from_numpy(np.array(invs, dtype=np.float32)).to(dev)
    pico_amd.dequant_segments(src.ptrs(), dst.ptrs(), fmt, inv_scales=inv, ddtype=dtype, counts=src.counts)
    torch.cuda.synchronize()
    got, guards = dst.read(np.uint32 if dtype == "float" else np.uint16)
    assert guards and src.unchanged()
    plan = pico_amd.plan_quant([p or 0 for p in dst.ptrs()], [p or 0 for p in src.ptrs()], src.counts, dtype)
    assert {r[4] for r in plan} == {0, 1}, "both bodies run"
    for k, x in enumerate(data):
        want = F.dequant(x, fmt, dtype, np.float32(invs[k]))
        want = want.view(np.uint32) if dtype == "float" else want
        bad = np.nonzero(got[k] != want)[0]
        assert bad.size == 0, (dtype, fmt, k, bad[:4], x[bad[:4]], got[k][bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_round_trip_is_exact_on_fp8_values(dev, fmt):
    """float source, scale 1: dequant(quant(x)) == x wherever x is an FP8 value"""
    codes = np.arange(256, dtype=np.uint8)
    codes = codes[~F.is_nan8(codes, fmt) & np.isfinite(F.decode(codes, fmt))]
    x = np.tile(F.decode(codes, fmt), 40)
    src = Bucket(4, [(x.size, 4, False)], [x])
    mid = Bucket(1, [(x.size, 1, False)])
    back = Bucket(4, [(x.size, 8, False)])
    pico_amd.quant_segments(src.ptrs(), mid.ptrs(), fmt, sdtype="float", counts=[x.size])
    pico_amd.dequant_segments(mid.ptrs(), back.ptrs(), fmt, ddtype="float", counts=[x.size])
    torch.cuda.synchronize()
    (q,), g1 = mid.read()
    (r,), g2 = back.read(np.uint32)
    assert g1 and g2
    assert np.array_equal(q, np.tile(codes, 40))
    assert np.array_equal(r, x.view(np.uint32))


# ---- bine_quant_multi ---------------------------------------------------------------------------------

SHARDS = [2048 * 4 + 5, 0, 37]


class Ranks:
    """per rank its shards (float32 masters) and the full FP8 tensors; rank k % P
    holds tensor k's largest magnitude"""

    def __init__(self, P, dtype, seed, nan_rank=None):
        self.P, self.dtype, self.n = P, dtype, len(SHARDS)
        rng = np.random.default_rng(seed)
        self.data = []
        for r in range(P):
            xs = [random_wide("float", c, rng) for c in SHARDS]
            for k, x in enumerate(xs):
                if x.size:
                    np.clip(x, -1000.0, 1000.0, out=x)
                    if r == k % P:
                        x[x.size // 2] = -4321.0 * (k + 1)
                    if r == nan_rank and k == 0:
                        x[3] = np.nan
            self.data.append([from_values(dtype, x) for x in xs])
        esz = ESZ[dtype]
        self.src = [Bucket(esz, [(c, ((k + 1) % 4) * esz, c == 0) for k, c in enumerate(SHARDS)], self.data[r])
                    for r in range(P)]
        self.p8 = [Bucket(1, [(P * c, (3 * k + 1) % 8, c == 0) for k, c in enumerate(SHARDS)]) for _ in range(P)]
        self.t, self.scales = zip(*[words(2 * self.n, dtype=torch.float32) for _ in range(P)])

    def state(self):
        return [(self.p8[r].t.cpu().numpy().tobytes(), self.scales[r].cpu().numpy().tobytes()) for r in range(self.P)]


@pytest.mark.parametrize("P", [2, 4])
def test_quant_multi_is_the_sim_and_its_five_parts(dev, P):
    cs = TG.comms(P)
    for dtype, fmt, ag in (("float", "e4m3", "ring"), ("bfloat16", "e5m2", "recursivedoubling")):
        fused, parts = Ranks(P, dtype, 41), Ranks(P, dtype, 41)
        rc, st = pico_amd.loopback_quant_multi(cs, "recursivedoubling", ag, [b.ptrs() for b in fused.p8],
                                               [b.ptrs() for b in fused.src], fmt, list(fused.scales), sdtype=dtype,
                                               shard_counts=SHARDS)
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * P, (rc, st)
        want8, want_scales = F.quant_multi(fused.data, dtype, fmt)
        for k in (0, 2):                          # the maximum sits on one rank alone
            assert F.amax_bits(fused.data[k % P][k], dtype) > max(
                F.amax_bits(fused.data[r][k], dtype) for r in range(P) if r != k % P)
        for r in range(P):
            got, guards = fused.p8[r].read()
            assert guards and fused.src[r].unchanged() and guards_ok(fused.t[r], 2 * fused.n)
            assert fused.scales[r].cpu().numpy().tobytes() == want_scales.tobytes(), r
            for k in range(fused.n):
                assert np.array_equal(got[k], want8[k]), (dtype, fmt, r, k)
        # the five public calls one by one
        n = parts.n
        vt, V = zip(*[words(n) for _ in range(P)])
        for r in range(P):
            pico_amd.amax_segments(parts.src[r].ptrs(), dtype=dtype, counts=SHARDS, out=V[r])
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allreduce(cs, "recursivedoubling", [pico_amd.IN_PLACE] * P, list(V), n, "uint32",
                                             "max")
        assert rc == 0 and st == [0] * P
        for r in range(P):
            pico_amd.fp8_scales(V[r], fmt, n=n, scales=parts.scales[r])
            slot = [None if c == 0 else a + r * c for a, c in zip(parts.p8[r].ptrs(), SHARDS)]
            pico_amd.quant_segments(parts.src[r].ptrs(), slot, fmt, scales=parts.scales[r], sdtype=dtype,
                                    counts=SHARDS)
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allgather_multi(cs, ag, None, [b.ptrs() for b in parts.p8], "uint8",
                                                   shard_counts=SHARDS)
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * P
        assert fused.state() == parts.state(), (dtype, fmt)


@pytest.mark.parametrize("P", [2, 4])
def test_quant_multi_nan_on_one_rank_gives_scale_one_everywhere(dev, P):
    cs = TG.comms(P)
    R = Ranks(P, "float", 43, nan_rank=P - 1)
    rc, st = pico_amd.loopback_quant_multi(cs, "recursivedoubling", "ring", [b.ptrs() for b in R.p8],
                                           [b.ptrs() for b in R.src], "e4m3", list(R.scales), shard_counts=SHARDS)
    torch.cuda.synchronize()
    assert rc == 0 and st == [0] * P
    want8, want_scales = F.quant_multi(R.data, "float", "e4m3")
    assert want_scales[0] == 1.0 and want_scales[3] == 1.0 and want_scales[2] != 1.0
    for r in range(P):
        got, guards = R.p8[r].read()
        assert guards
        assert R.scales[r].cpu().numpy().tobytes() == want_scales.tobytes()
        assert all(np.array_equal(got[k], want8[k]) for k in range(R.n))
        assert got[0][(P - 1) * SHARDS[0] + 3] == 0x7F


def test_quant_multi_nothing_to_do(dev):
    cs = TG.comms(2)
    t, sc = zip(*[words(2, dtype=torch.float32) for _ in range(2)])
    rc, st = pico_amd.loopback_quant_multi(cs, "recursivedoubling", "ring", [[None], [None]], [[None], [None]], "e4m3",
                                           list(sc), sdtype="float", shard_counts=[0])
    torch.cuda.synchronize()
    assert rc == 0 and st == [0, 0]
    assert all(guards_ok(x, 0) for x in t), "B = 0 writes nothing, scales included"
