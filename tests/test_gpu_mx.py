"""MX block-scaled quantization on the GPU: bine_mx_quant_segments and
bine_mx_dequant_segments against tests/mx_sim.py, the numpy statement of the
header's contract, bit for bit on both bodies, and bine_mx_quant_multi over
loopback ranks against the sim's two steps, against the two public calls issued
one by one and against the sim on the whole tensor.  Guard bytes surround every
output and every source is compared untouched.  (Real processes and graph
mode: tools/mx_check.py, tests/test_gpu_mx_rccl.py.)"""
import numpy as np
import pytest

import fp8_sim as F
import h16_util as H
import mx_sim as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd import _lib  # noqa: E402
from test_gpu_quant import Bucket, from_values  # noqa: E402  (the guarded arena)

S = _lib.MX_SEGS_PER_LAUNCH
ESZ = {"float": 4, "float16": 2, "bfloat16": 2}
TYPES = sorted(ESZ)
CASES = [(d, f) for d in TYPES for f in M.FORMATS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tile_of(dtype):
    return 32768 // ESZ[dtype]


def to_wide(dtype, bits32):
    """binary32 patterns -> the type's elements (16-bit types: the upper half for
    bfloat16, the nearest float16)"""
    bits32 = np.ascontiguousarray(bits32, dtype=np.uint32)
    if dtype == "float":
        return bits32.view(np.float32).copy()
    if dtype == "bfloat16":
        return (bits32 >> np.uint32(16)).astype(np.uint16)
    return H.from_f32(bits32.view(np.float32), dtype)


# ---- inputs --------------------------------------------------------------------------------

def random_blocks(dtype, n, rng):
    """each block in a binade range of its own, elements up to 40 binades below the block's top,
    signs, a few zeros"""
    nb = M.nblk(n)
    lo, hi = (-24, 15) if dtype == "float16" else (-140, 127)
    top = np.repeat(rng.integers(lo, hi, nb), 32)[:n]
    x = rng.standard_normal(n) * np.exp2(top - rng.integers(0, 40, n) * (rng.integers(0, 3, n) == 0))
    x[rng.integers(0, 11, n) == 0] = 0.0
    with np.errstate(over="ignore", under="ignore"):
        return from_values(dtype, x.astype(np.float32))


def all_patterns(dtype):
    """all 65,536 16-bit patterns (float: as the upper half of a binary32), 31 to
    a block behind a leader of larger or equal magnitude: the chunk's largest
    finite magnitude lifted by 0 to 33 binades, so the 31 fall anywhere from the
    block's top binade down to below the format's smallest subnormal"""
    pats = np.arange(1 << 16, dtype=np.uint32)
    order = np.argsort(((pats & 0x7FFF) << 1) | (pats >> 15), kind="stable")
    pats = pats[order]
    lifts = (0, 1, 2, 5, 8, 9, 10, 14, 15, 16, 17, 18, 19, 29, 30, 31, 32, 33)
    ebits, mbits = (5, 10) if dtype == "float16" else (8, 7)
    emax_field = (1 << ebits) - 2
    out = []
    for j, at in enumerate(range(0, pats.size, 31)):
        chunk = pats[at:at + 31]
        mag = int((chunk & 0x7FFF).max())
        ex = min(mag >> mbits, emax_field)
        lead = (min(ex + lifts[j % len(lifts)], emax_field) << mbits) | (mag & ((1 << mbits) - 1) if ex == mag >> mbits
                                                                         else (1 << mbits) - 1)
        out.append(np.concatenate([[lead | ((j & 1) << 15)], chunk]))
    p = np.concatenate(out).astype(np.uint32)
    if dtype == "float":
        return (p << np.uint32(16)).view(np.float32)
    return p.astype(np.uint16)


def midpoint_blocks(dtype, fmt):
    """every midpoint between neighbouring codes, the values one ulp either side,
    the codes and values between FMAX and 2^(emax + 1), at three block exponents:
    31 to a block behind the leader 1.5 * 2^emax * 2^k"""
    pts = M.midpoints(fmt).astype(np.float64)
    out = []
    for k in ((-10, -4, 0) if dtype == "float16" else (-100, 0, 90)):
        for at in range(0, pts.size, 31):
            out.append(np.concatenate([[1.5 * 2.0 ** M.EMAX[fmt]], pts[at:at + 31]]) * 2.0 ** k)
    with np.errstate(over="ignore", under="ignore"):
        return from_values(dtype, np.concatenate(out).astype(np.float32))


def special_blocks(dtype, rng):
    """block by block: a float32-subnormal maximum (S = 0), a small normal
    maximum that still gives S = 0, a maximum near the type's largest value,
    zeros with -0 among them, one NaN, one infinity, both, and random blocks
    between them"""
    big = 65504.0 if dtype == "float16" else 3.4028234e38
    tiny_bits = np.concatenate([np.arange(1, 17), [0x7FFFFF, 0x400000, 0x80000001, 0x807FFFFF], np.arange(3, 15) << 16])
    blocks = [to_wide(dtype, tiny_bits.astype(np.uint32)),
              from_values(dtype, np.ldexp(rng.standard_normal(32), -125 if dtype != "float16" else -20)),
              from_values(dtype, np.concatenate([[big, -big / 3, big / 2 ** 9, -big / 2 ** 17], rng.standard_normal(28)])),
              from_values(dtype, [0.0, -0.0] * 16),
              from_values(dtype, [-0.0] * 32)]
    for bad in ([np.nan], [np.inf], [-np.inf, np.nan]):
        x = rng.standard_normal(32)
        x[rng.choice(32, len(bad), replace=False)] = bad
        blocks.append(from_values(dtype, x))
    mixed = []
    for b in blocks:
        assert b.size == 32
        mixed += [b, random_blocks(dtype, 32, rng)]
    return np.concatenate(mixed)


def segments_of(dtype, fmt, rng):
    tile = tile_of(dtype)
    segs = [all_patterns(dtype), midpoint_blocks(dtype, fmt), special_blocks(dtype, rng)]
    segs += [random_blocks(dtype, c, rng) for c in (1, 31, 32, 33, tile - 1, tile, tile + 1, 2 * tile + 17)]
    if fmt == "e2m1":
        segs += [random_blocks(dtype, c, rng) for c in (3, 63, 65)]          # odd counts: the last byte's high nibble
    return segs


def run_quant(dtype, fmt, data, sphase, dphases):
    """quantize `data` (a list of segments) with every source `sphase` elements off a 16-B boundary and the data
    bytes at the cycling `dphases`; returns (data bytes, scale bytes) per segment, everything else checked"""
    esz = ESZ[dtype]
    counts = [x.size for x in data]
    src = Bucket(esz, [(c, sphase * esz, False) for c in counts], data)
    d8 = Bucket(1, [(M.dbytes(c, fmt), dphases[k % len(dphases)], False) for k, c in enumerate(counts)])
    sc = Bucket(1, [(M.nblk(c), (5 * k + sphase) % 7, False) for k, c in enumerate(counts)])
    plan = pico_amd.plan_mx(src.ptrs(), d8.ptrs(), sc.ptrs(), counts, dtype, fmt)
    pico_amd.mx_quant_segments(src.ptrs(), d8.ptrs(), sc.ptrs(), fmt, sdtype=dtype, counts=counts)
    torch.cuda.synchronize()
    q, g1 = d8.read()
    s, g2 = sc.read()
    assert g1 and g2, "bytes outside the outputs were written"
    assert src.unchanged(), "a source was written"
    return q, s, plan


def assert_is_sim(dtype, fmt, data, q, s, what):
    for k, x in enumerate(data):
        wq, ws = M.quant(x, dtype, fmt)
        bad = np.nonzero(s[k] != ws)[0]
        assert bad.size == 0, (what, dtype, fmt, k, "scales", bad[:4], s[k][bad[:4]], ws[bad[:4]])
        bad = np.nonzero(q[k] != wq)[0]
        assert bad.size == 0, (what, dtype, fmt, k, "data", bad[:4], q[k][bad[:4]], wq[bad[:4]])


# ---- bine_mx_quant_segments ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,fmt", CASES)
def test_quant_is_the_sim_on_both_bodies(dev, dtype, fmt):
    rng = np.random.default_rng(320)
    data = segments_of(dtype, fmt, rng)
    # what the inputs are meant to hold, checked on the sim's scale bytes
    sp = M.block_scales(special_blocks(dtype, np.random.default_rng(1)), dtype, fmt)
    assert (sp[[10, 12, 14]] == 0xFF).all() and sp[6] == 0 and sp[8] == 0
    assert sp[0] == 0 or dtype == "float16"                      # a float32-subnormal maximum
    q, s, plan = run_quant(dtype, fmt, data, 0, (0,))
    assert all(r[4] == 0 for r in plan)                          # the vector body
    assert_is_sim(dtype, fmt, data, q, s, "vector")
    q, s, plan = run_quant(dtype, fmt, data, 1, (1, 2, 3))
    assert all(r[4] == 1 for r in plan)                          # the element body
    assert_is_sim(dtype, fmt, data, q, s, "element")


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_clamp_and_top_binade(dev, fmt):
    """block maxima between FMAX and 2^(emax + 1) keep S and saturate"""
    top, lim = M.FMAX[fmt], 2.0 ** (M.EMAX[fmt] + 1)
    x = np.zeros(64, dtype=np.float32)
    x[0], x[1], x[2] = np.nextafter(np.float32(top), np.float32(np.inf)), -(top + lim) / 2, 1.0
    x[32], x[33] = np.nextafter(np.float32(lim), np.float32(0)), -top
    q, s, _ = run_quant("float", fmt, [x], 0, (0,))
    assert s[0].tolist() == [127, 127]
    codes = M.unpack(q[0], 64, fmt)
    fmax_code = {"e4m3": 0x7E, "e5m2": 0x7B, "e2m1": 7}[fmt]
    neg = 8 if fmt == "e2m1" else 0x80
    assert codes[[0, 1, 32, 33]].tolist() == [fmax_code, fmax_code | neg, fmax_code, fmax_code | neg]
    assert_is_sim("float", fmt, [x], q, s, "clamp")


# ---- bine_mx_dequant_segments ------------------------------------------------------------------------

SCALES = (0, 1, 126, 127, 128, 254, 255)


@pytest.mark.parametrize("dtype,fmt", CASES)
def test_dequant_is_the_sim_on_both_bodies(dev, dtype, fmt):
    """all 256 data bytes (16 nibbles in both positions) under seven scale bytes, two tiles + 17 elements"""
    esz = ESZ[dtype]
    n = 2 * tile_of(dtype) + 17
    i = np.arange(n)
    if fmt == "e2m1":
        codes = ((i + i // 32) % 16).astype(np.uint8)
        assert {(int(c), int(p)) for c, p in zip(codes[:1024], i[:1024] & 1)} == {(c, p) for c in range(16) for p in (0, 1)}
    else:
        codes = (i % 256).astype(np.uint8)
    data = M.pack(codes, fmt)
    sb = np.array(SCALES, dtype=np.uint8)[(np.arange(M.nblk(n)) // 8) % len(SCALES)]
    want = M.dequant(data, sb, n, fmt, dtype)
    view = np.uint32 if dtype == "float" else np.uint16
    for sphase, dphase, body in ((0, 0, 0), (1, 1, 1), (1, 3, 1)):
        d8 = Bucket(1, [(data.size, dphase, False)], [data])
        sc = Bucket(1, [(sb.size, 3 * dphase, False)], [sb])
        dst = Bucket(esz, [(n, sphase * esz, False)])
        assert [r[4] for r in pico_amd.plan_mx(dst.ptrs(), d8.ptrs(), sc.ptrs(), [n], dtype, fmt)] == [body]
        pico_amd.mx_dequant_segments(d8.ptrs(), sc.ptrs(), dst.ptrs(), fmt, ddtype=dtype, counts=[n])
        torch.cuda.synchronize()
        (got,), guards = dst.read(view)
        assert guards and d8.unchanged() and sc.unchanged()
        bad = np.nonzero(got != want.view(view))[0]
        assert bad.size == 0, (dtype, fmt, body, bad[:4], codes[bad[:4]], sb[bad[:4] // 32], got[bad[:4]],
                               want.view(view)[bad[:4]])


# ---- lists ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, S + 1])
def test_lists_with_empties(dev, n):
    rng = np.random.default_rng(n)
    for dtype, fmt in (("float", "e4m3"), ("bfloat16", "e2m1"), ("float16", "e5m2")):
        esz = ESZ[dtype]
        counts = [0 if k % 5 == 2 else int(rng.integers(1, 200)) for k in range(n)]
        data = [random_blocks(dtype, c, rng) for c in counts]
        null = [c == 0 and k % 2 == 0 for k, c in enumerate(counts)]
        src = Bucket(esz, [(c, (k % 3 == 1) * esz, null[k]) for k, c in enumerate(counts)], data)
        d8 = Bucket(1, [(M.dbytes(c, fmt), (k % 3 == 2) * (1 + k % 3), null[k]) for k, c in enumerate(counts)])
        sc = Bucket(1, [(M.nblk(c), k % 4, null[k]) for k, c in enumerate(counts)])
        plan = pico_amd.plan_mx([p or 0 for p in src.ptrs()], [p or 0 for p in d8.ptrs()], [p or 0 for p in sc.ptrs()],
                                counts, dtype, fmt)
        assert len(plan) == sum(c > 0 for c in counts) and len({r[0] for r in plan}) == -(-len(plan) // S)
        assert n < 2 or {r[4] for r in plan} == {0, 1}
        pico_amd.mx_quant_segments(src.ptrs(), d8.ptrs(), sc.ptrs(), fmt, sdtype=dtype, counts=counts)
        torch.cuda.synchronize()
        q, g1 = d8.read()
        s, g2 = sc.read()
        assert g1 and g2 and src.unchanged()
        assert_is_sim(dtype, fmt, data, q, s, "list")
        # and back: the same lists the other way round
        back = Bucket(esz, [(c, (k % 3 == 1) * esz, null[k]) for k, c in enumerate(counts)])
        pico_amd.mx_dequant_segments(d8.ptrs(), sc.ptrs(), back.ptrs(), fmt, ddtype=dtype, counts=counts)
        torch.cuda.synchronize()
        view = np.uint32 if dtype == "float" else np.uint16
        got, g3 = back.read(view)
        assert g3
        for k, c in enumerate(counts):
            assert np.array_equal(got[k], M.dequant(q[k], s[k], c, fmt, dtype).view(view)), (dtype, fmt, k)


# ---- bine_mx_quant_multi ---------------------------------------------------------------------------------

SHARDS = [32, 8192 + 32, 0]


class Ranks:
    """per rank its shards, the full tensors' data bytes and their scale bytes;
    tensor 0 takes the element body, tensor 1 (a full tile and a block) the vector body"""

    def __init__(self, P, dtype, fmt, seed):
        self.P, self.n = P, len(SHARDS)
        rng = np.random.default_rng(seed)
        self.data = [[random_blocks(dtype, c, rng) for c in SHARDS] for _ in range(P)]
        esz = ESZ[dtype]
        self.src = [Bucket(esz, [(c, (k == 0) * esz, c == 0) for k, c in enumerate(SHARDS)], self.data[r])
                    for r in range(P)]
        self.p8 = [Bucket(1, [(P * M.dbytes(c, fmt), (k == 0) * 3, c == 0) for k, c in enumerate(SHARDS)])
                   for _ in range(P)]
        self.s8 = [Bucket(1, [(P * (c // 32), (k + 1) % 4, c == 0) for k, c in enumerate(SHARDS)]) for _ in range(P)]

    def state(self):
        return [(self.p8[r].t.cpu().numpy().tobytes(), self.s8[r].t.cpu().numpy().tobytes()) for r in range(self.P)]


@pytest.mark.parametrize("P", [2, 4])
def test_mx_quant_multi_is_the_sim_its_two_parts_and_the_whole_tensor(dev, P):
    cs = TG.comms(P)
    for dtype, fmt, ag in (("float", "e4m3", "ring"), ("bfloat16", "e2m1", "recursivedoubling"),
                           ("float16", "e5m2", "ring")):
        fused, parts = Ranks(P, dtype, fmt, 47), Ranks(P, dtype, fmt, 47)
        rc, st = pico_amd.loopback_mx_quant_multi(cs, ag, [b.ptrs() for b in fused.p8], [b.ptrs() for b in fused.s8],
                                                  [b.ptrs() for b in fused.src], fmt, sdtype=dtype,
                                                  shard_counts=SHARDS)
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * P, (rc, st)
        want8, wants = M.quant_multi(fused.data, dtype, fmt)
        for r in range(P):
            got8, g1 = fused.p8[r].read()
            gots, g2 = fused.s8[r].read()
            assert g1 and g2 and fused.src[r].unchanged()
            for k in range(fused.n):
                assert np.array_equal(got8[k], want8[k]) and np.array_equal(gots[k], wants[k]), (dtype, fmt, r, k)
        # the whole tensor's blocks: the sim on the concatenation of the shards
        for k, c in enumerate(SHARDS):
            if c:
                whole = np.concatenate([fused.data[r][k] for r in range(P)])
                wq, ws = M.quant(whole, dtype, fmt)
                assert np.array_equal(want8[k], wq) and np.array_equal(wants[k], ws)
        # the two public calls one by one
        for r in range(P):
            d = [None if c == 0 else a + r * M.dbytes(c, fmt) for a, c in zip(parts.p8[r].ptrs(), SHARDS)]
            s = [None if c == 0 else a + r * (c // 32) for a, c in zip(parts.s8[r].ptrs(), SHARDS)]
            pico_amd.mx_quant_segments(parts.src[r].ptrs(), d, s, fmt, sdtype=dtype, counts=SHARDS)
        torch.cuda.synchronize()
        rc, st = pico_amd.loopback_allgather_multi(
            cs, ag, None, [parts.p8[r].ptrs() + parts.s8[r].ptrs() for r in range(P)], "uint8",
            shard_counts=[M.dbytes(c, fmt) for c in SHARDS] + [c // 32 for c in SHARDS])
        torch.cuda.synchronize()
        assert rc == 0 and st == [0] * P
        assert fused.state() == parts.state(), (dtype, fmt)


def test_mx_quant_multi_nothing_to_do(dev):
    cs = TG.comms(2)
    rc, st = pico_amd.loopback_mx_quant_multi(cs, "ring", [[None], [None]], [[None], [None]], [[None], [None]], "e4m3",
                                              sdtype="float", shard_counts=[0])
    assert rc == 0 and st == [0, 0]
    rc, st = pico_amd.loopback_mx_quant_multi(cs, "ring", [[]] * 2, [[]] * 2, [[]] * 2, "e2m1", sdtype="float",
                                              shard_counts=[])
    assert rc == 0 and st == [0, 0]
