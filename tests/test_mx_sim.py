"""tests/mx_sim.py pinned: the FP8 element encoding to fp8_sim.encode (itself
pinned to torch), the E2M1 encoding to the 16-value table by brute force in
float64, the scale byte to math.frexp, the E8M0 bytes to torch.float8_e8m0fnu,
and the point of the rule: a block's scaled maximum lies in [2^emax,
2^(emax+1)).  No GPU, no native code."""
import math

import numpy as np
import pytest
import torch

import fp8_sim as F
import mx_sim as M


def f32(v):
    return np.array(v, dtype=np.float32)


@pytest.mark.parametrize("fmt", ("e4m3", "e5m2"))
def test_fp8_encoding_is_fp8_sims(fmt):
    y = np.concatenate([M.midpoints(fmt), F.midpoints(fmt)])
    y = y[~np.isnan(y)]
    assert np.array_equal(M.encode(y, fmt), F.encode(y, fmt))
    q, S = M.quant(f32([1.0] + [0.0] * 31), "float", fmt)       # a block whose maximum is 1: S = 127 - emax
    assert S.tolist() == [127 - M.EMAX[fmt]] and q[0] == F.encode(f32([2.0 ** M.EMAX[fmt]]), fmt)[0]


def nearest_even_e2m1(y: float) -> int:
    """brute force in float64: the nearest of the 8 magnitudes, a tie to the even code"""
    a = min(abs(y), 6.0)
    best = min(range(8), key=lambda m: (abs(M.E2M1_VALUES[m] - a), m & 1))
    return best | (8 if math.copysign(1.0, y) < 0 else 0)


def test_e2m1_encoding_against_the_table():
    v = np.array(M.E2M1_VALUES)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)
    pts = np.concatenate([mid, np.nextafter(mid, f32(np.inf)), np.nextafter(mid, f32(-np.inf)), v.astype(np.float32),
                          f32([6.0, 6.5, 7.999, 1e-45, 2.0 ** -127, 0.2499999, 1e30, np.inf]),
                          np.linspace(0, 8, 4097, dtype=np.float32)])
    pts = np.concatenate([pts, -pts]).astype(np.float32)
    got = M.encode(pts, "e2m1")
    want = [nearest_even_e2m1(float(y)) for y in pts]
    assert got.tolist() == want
    assert M.encode(f32([0.0, -0.0]), "e2m1").tolist() == [0, 8]
    # ties to the even code, spelled out: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    assert M.decode_e2m1(M.encode(f32([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]), "e2m1")).tolist() == \
        [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert M.decode_e2m1(np.arange(16, dtype=np.uint8)).tolist() == list(M.E2M1_VALUES) + [-x for x in M.E2M1_VALUES]


def test_e2m1_packing():
    c = np.array([1, 2, 3, 15, 7], dtype=np.uint8)
    p = M.pack(c, "e2m1")
    assert p.tolist() == [0x21, 0xF3, 0x07]                     # element 2j in the low nibble; the odd end's high nibble 0
    assert M.unpack(p, 5, "e2m1").tolist() == c.tolist()
    assert M.dbytes(5, "e2m1") == 3 and M.dbytes(5, "e4m3") == 5 and M.nblk(33) == 2 and M.nblk(32) == 1


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_scale_byte_against_frexp(fmt):
    for bits in M.scale_patterns():
        S = M.scale_byte(bits, fmt)
        if bits >= 0x7F800000:
            assert S == 0xFF
            continue
        if bits == 0:
            assert S == 0
            continue
        a = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
        m, x = math.frexp(a)                                     # a = m * 2^x, m in [0.5, 1)
        floor_log2 = x - 1
        assert S == max(floor_log2 - M.EMAX[fmt] + 127, 0) and S <= 252
        if S > 0:
            assert S - 127 + M.EMAX[fmt] == floor_log2


def test_scale_bytes_are_e8m0():
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    v = b.view(torch.float8_e8m0fnu).to(torch.float32).numpy()
    assert np.isnan(v[255])
    want = np.ldexp(np.float32(1.0), np.arange(255, dtype=np.int32) - 127).astype(np.float32)
    assert v[:255].tobytes() == want.tobytes()


def generated_blocks(dtype):
    rng = np.random.default_rng(32)
    pats = rng.integers(0, 1 << 32, 32 * 4000, dtype=np.uint64).astype(np.uint32)
    if dtype == "float":
        return pats.view(np.float32)
    return (pats >> np.uint32(16)).astype(np.uint16)


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("dtype", M.WIDE)
def test_scaled_maximum_fills_the_top_binade(dtype, fmt):
    x = generated_blocks(dtype)
    S = M.block_scales(x, dtype, fmt)
    with np.errstate(invalid="ignore"):                          # signalling NaNs among the random patterns
        a = np.abs(F.widen(x, dtype).astype(np.float64)).reshape(-1, 32)
    seen = 0
    for b in range(S.size):
        if not np.all(np.isfinite(a[b])) or S[b] == 0:           # S = 0: the maximum is too small to be lifted further
            assert S[b] in (0, 0xFF)
            continue
        top = a[b].max() * 2.0 ** (127 - int(S[b]))
        assert 2.0 ** M.EMAX[fmt] <= top < 2.0 ** (M.EMAX[fmt] + 1)
        seen += 1
    assert seen > 1000


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_round_trip_and_special_blocks(fmt):
    x = np.zeros(96, dtype=np.float32)
    x[0:32] = np.linspace(-3, 5, 32)
    x[40] = np.nan                                               # block 1: S = 0xFF, data 0
    x[64:96] = -0.0                                              # block 2: all zero, S = 0, the sign kept
    q, S = M.quant(x, "float", fmt)
    assert S.tolist() == [127 + 2 - M.EMAX[fmt], 0xFF, 0]
    codes = M.unpack(q, 96, fmt)
    assert not codes[32:64].any() and set(codes[64:96].tolist()) == {8 if fmt == "e2m1" else 0x80}
    y = M.dequant(q, S, 96, fmt, "float")
    assert np.isnan(y[32:64]).all() and y[32:64].view(np.uint32).tolist() == [0x7FC00000] * 32
    assert np.array_equal(y[64:96].view(np.uint32), x[64:96].view(np.uint32))
    assert np.max(np.abs(y[:32] - x[:32])) <= (1.0 if fmt == "e2m1" else 0.5)
    # the clamp acts: 500 alone in a block scales to itself (E = 8) and gives 448 in e4m3
    if fmt == "e4m3":
        q, S = M.quant(f32([500.0]), "float", fmt)
        assert S.tolist() == [127] and M.dequant(q, S, 1, fmt, "float").tolist() == [448.0]
