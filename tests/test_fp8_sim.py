"""tests/fp8_sim.py against torch's CPU float8 types (no GPU, no library call):
the sim is what every FP8 test compares the kernels with, so it is pinned here
to an independent implementation of the OCP encodings.

torch rounds to nearest even, subnormals included (17 -> 16, 19 -> 20, 2^-10 ->
0, 1.5 * 2^-10 -> 2^-9 in e4m3).  A NaN input is excepted: the contract maps it
to the byte 0x7F whatever its sign.
"""
import numpy as np
import pytest
import torch

import fp8_sim as F
import h16_util as H

TORCH8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def torch_encode(y, fmt):
    """clamp, then torch's conversion, as bytes"""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    return torch.clamp(t, -F.FMAX[fmt], F.FMAX[fmt]).to(TORCH8[fmt]).view(torch.uint8).numpy()


def check_encode(y, fmt):
    y = np.ascontiguousarray(y, dtype=np.float32)
    got = F.encode(y, fmt)
    nan = np.isnan(y)
    assert (got[nan] == 0x7F).all()
    want = torch_encode(y[~nan], fmt)
    bad = np.nonzero(got[~nan] != want)[0]
    assert bad.size == 0, (fmt, y[~nan][bad[:5]], got[~nan][bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_torch_rounds_ties_to_even(fmt):
    if fmt == "e4m3":
        y = np.array([17, 19, 2.0 ** -10, 1.5 * 2.0 ** -10], dtype=np.float32)
        want = [16, 20, 0, 2.0 ** -9]
    else:
        y = np.array([9, 11, 2.0 ** -17, 1.5 * 2.0 ** -17], dtype=np.float32)
        want = [8, 12, 0, 2.0 ** -16]
    got = torch.from_numpy(torch_encode(y, fmt)).view(TORCH8[fmt]).to(torch.float32).numpy()
    assert got.tolist() == want


@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3, 2.0 ** 5])
def test_encode_all_16bit_patterns(dtype, fmt, scale):
    with np.errstate(all="ignore"):
        y = F.widen(F.all16(dtype), dtype) * np.float32(scale)
    check_encode(y, fmt)
    assert np.array_equal(F.quant(F.all16(dtype), dtype, fmt, scale), F.encode(y, fmt))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_encode_midpoints(fmt):
    y = F.midpoints(fmt)
    assert y.size > 6 * 100
    check_encode(y, fmt)
    # -0 keeps its sign, +-inf saturates, the clamp holds FMAX
    top = 0x7E if fmt == "e4m3" else 0x7B
    assert F.encode(np.array([-0.0, 0.0, np.inf, -np.inf, 1e30], dtype=np.float32), fmt).tolist() == \
        [0x80, 0x00, top, 0x80 | top, top]


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_decode_all_bytes(fmt):
    b = np.arange(256, dtype=np.uint8)
    got = F.decode(b, fmt)
    want = torch.from_numpy(b).view(TORCH8[fmt]).to(torch.float32).numpy()
    nan = F.is_nan8(b, fmt)
    assert np.array_equal(np.isnan(want), nan) and np.isnan(got[nan]).all()
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    # the contract's NaN: quiet, the byte's sign
    assert set(got[nan].view(np.uint32).tolist()) == {0x7FC00000, 0xFFC00000}
    # every finite byte survives the round trip (e5m2's infinities saturate)
    fin = np.isfinite(got)
    assert np.array_equal(F.encode(got[fin], fmt), b[fin])


@pytest.mark.parametrize("dtype", H.TYPES)
def test_widen_bits_is_exact(dtype):
    b = F.all16(dtype)
    nan = H.is_nan(b, dtype)
    assert np.array_equal(F.widen(b, dtype)[~nan].view(np.uint32), H.to_f32(b, dtype)[~nan].view(np.uint32))
    w = F.widen_bits(b, dtype)
    assert ((w[nan] & 0x7FFFFFFF) > 0x7F800000).all()
    # a NaN keeps its sign and payload: the smallest signalling payload stays signalling
    one = np.array([0x7C01 if dtype == "float16" else 0x7F81], dtype=np.uint16)
    assert F.widen_bits(one, dtype)[0] == (0x7F802000 if dtype == "float16" else 0x7F810000)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_scale_rule_properties(fmt):
    for bits in F.boundary_patterns(fmt):
        s, i = F.scale_rule(bits, fmt)
        e = F.scale_exp(bits, fmt)
        assert float(s) * float(i) == 1.0
        if bits == 0 or bits >= 0x7F800000:
            assert e == 0
            continue
        a = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
        if -126 < e < 126:
            assert a * float(s) <= F.FMAX[fmt] < a * 2 * float(s), hex(bits)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_quant_multi_sim(fmt):
    rng = np.random.default_rng(5)
    src = [[rng.standard_normal(c).astype(np.float32) * (r + 1) for c in (5, 0, 9)] for r in range(2)]
    p8, scales = F.quant_multi(src, "float", fmt)
    assert [p.size for p in p8] == [10, 0, 18] and scales.size == 6
    amax = max(np.abs(src[0][0]).max(), np.abs(src[1][0]).max())
    assert amax * scales[0] <= F.FMAX[fmt] < 2 * amax * scales[0]
    assert scales[1] == 1.0 and scales[4] == 1.0                 # the empty tensor
    back = F.dequant(p8[2][9:], fmt, "float", scales[5])
    assert np.abs(back - src[1][2]).max() <= np.abs(src[1][2]).max() * 2.0 ** -(F.MB[fmt])
