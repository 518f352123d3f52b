"""The MX block-scaled quantization contract of include/bine_amd.h restated in
numpy, one operation per line (test infrastructure).

Wide data lives on the host as in tests/fp8_sim.py: float32 arrays ("float")
or uint16 bit patterns ("float16", "bfloat16").  A segment is cut into blocks
of 32 elements from its first element; the last may be short.

  scale_byte   the E8M0 byte of a block from the pattern of its largest
               magnitude, with frexp: S - 127 + emax = floor(log2 amax)
  encode       y -> data code: the FP8 bytes are fp8_sim.encode's; E2M1 is the
               clamp to +-6 and round to nearest even on the integer fields
  decode       the code's value, exactly
  quant / dequant / quant_multi   the entry points' statements
"""
import numpy as np

import fp8_sim as F
import h16_util as H

FORMATS = ("e4m3", "e5m2", "e2m1")
EMAX = {"e4m3": 8, "e5m2": 15, "e2m1": 2}
FMAX = {"e4m3": 448.0, "e5m2": 57344.0, "e2m1": 6.0}
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # the magnitude of code m
BLOCK = 32
WIDE = F.WIDE
NP_WIDE = F.NP_WIDE


def dbytes(count: int, fmt: str) -> int:
    return (count + 1) // 2 if fmt == "e2m1" else count


def nblk(count: int) -> int:
    return (count + BLOCK - 1) // BLOCK


def scale_bytes(A, fmt: str):
    """A = per block the largest bits(widen(x)) & 0x7fffffff (uint32) -> S (uint8)"""
    A = np.ascontiguousarray(A, dtype=np.uint32)
    finite = np.where(A >= np.uint32(0x7F800000), np.uint32(0), A).astype(np.uint32)
    f, x = np.frexp(finite.view(np.float32).astype(np.float64))   # a = f * 2^x, f in [0.5, 1): floor(log2 a) = x - 1
    S = np.maximum(x.astype(np.int64) - 1 - EMAX[fmt] + 127, 0)
    S = np.where(A == 0, 0, S)
    return np.where(A >= np.uint32(0x7F800000), 0xFF, S).astype(np.uint8)


def scale_byte(bits: int, fmt: str) -> int:
    return int(scale_bytes(np.array([bits], dtype=np.uint32), fmt)[0])


def encode_e2m1(y):
    """float32 values (no NaN) -> E2M1 codes 0..15"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    c = np.minimum(np.maximum(y, np.float32(-6.0)), np.float32(6.0))
    u = c.view(np.uint32).astype(np.uint64)
    sign = (u >> np.uint64(31)) << np.uint64(3)
    a = u & np.uint64(0x7FFFFFFF)
    ef = a >> np.uint64(23)
    # the format's normal range (>= 1): drop 22 fraction bits, nearest even, then rebase the exponent (bias 1)
    sh = np.uint64(22)
    lsb = (a >> sh) & np.uint64(1)
    rn = (a + ((np.uint64(1) << (sh - np.uint64(1))) - np.uint64(1)) + lsb) >> sh
    normal = rn - np.uint64(126 << 1)
    # below it: the value in units of the subnormal 0.5, nearest even
    e1 = np.maximum(ef, np.uint64(1))
    sig = np.where(ef > 0, (a & np.uint64(0x7FFFFF)) | np.uint64(0x800000), a & np.uint64(0x7FFFFF))
    s = np.minimum(np.uint64(149) - e1, np.uint64(40))        # value = sig * 2^(e1 - 150) = (sig >> s) * 0.5
    q = sig >> s
    rem = sig & ((np.uint64(1) << s) - np.uint64(1))
    half = np.uint64(1) << (s - np.uint64(1))
    up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
    sub = q + up.astype(np.uint64)
    code = np.where(ef >= np.uint64(127), normal, sub)
    return (sign | code).astype(np.uint8)


def encode(y, fmt):
    """float32 values (no NaN) -> data codes: bytes, or nibbles for e2m1"""
    return encode_e2m1(y) if fmt == "e2m1" else F.encode(y, fmt)


def decode_e2m1(c):
    c = np.ascontiguousarray(c, dtype=np.uint8)
    v = np.array(E2M1_VALUES, dtype=np.float32)[c & np.uint8(7)]
    return np.where((c & np.uint8(8)) != 0, -v, v).astype(np.float32)


def pack(codes, fmt):
    """data codes -> data bytes: e2m1 two per byte, element 2j in the low nibble of byte j"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if fmt != "e2m1":
        return codes
    c = np.concatenate([codes, np.zeros(codes.size & 1, dtype=np.uint8)])
    return (c[0::2] | (c[1::2] << np.uint8(4))).astype(np.uint8)


def unpack(data, count, fmt):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if fmt != "e2m1":
        return data[:count]
    c = np.empty(2 * data.size, dtype=np.uint8)
    c[0::2] = data & np.uint8(15)
    c[1::2] = data >> np.uint8(4)
    return c[:count]


def block_scales(x, dtype, fmt):
    """the nblk scale bytes of one segment"""
    a = F.widen_bits(x, dtype) & np.uint32(0x7FFFFFFF)
    a = np.concatenate([a, np.zeros(-a.size % BLOCK, dtype=np.uint32)])       # a short last block: zeros change no maximum
    return scale_bytes(a.reshape(-1, BLOCK).max(axis=1), fmt) if a.size else np.zeros(0, dtype=np.uint8)


def quant(x, dtype, fmt):
    """(data bytes, scale bytes) of one segment"""
    S = block_scales(x, dtype, fmt)
    w = F.widen(x, dtype)
    per = np.repeat(S.astype(np.int64), BLOCK)[:w.size]                     # each element's scale byte
    dead = per == 0xFF
    factor = np.ldexp(np.float32(1.0), np.where(dead, 127, 127 - per).astype(np.int32)).astype(np.float32)
    with np.errstate(all="ignore"):
        y = (w * factor).astype(np.float32)           # one float32 multiplication
    tiny = np.abs(y) < np.float32(2.0 ** -126)        # below the normal range every format encodes a zero ...
    y = np.where(tiny, np.copysign(np.float32(0), y), y).astype(np.float32)     # ... of the product's sign
    y = np.where(dead, np.float32(0), y).astype(np.float32)
    codes = np.where(dead, np.uint8(0), encode(y, fmt)).astype(np.uint8)
    return pack(codes, fmt), S


def dequant(data, S, count, fmt, dtype):
    """the destination's elements: float32 values, or uint16 patterns"""
    codes = unpack(data, count, fmt)
    per = np.repeat(np.ascontiguousarray(S, dtype=np.uint8).astype(np.int64), BLOCK)[:count]
    dead = per == 0xFF
    inv = np.ldexp(np.float32(1.0), np.where(dead, 0, per - 127).astype(np.int32)).astype(np.float32)   # 2^-127: subnormal
    if fmt == "e2m1":
        d, nan = decode_e2m1(codes), np.zeros(count, dtype=bool)
    else:
        d, nan = F.decode(codes, fmt), F.is_nan8(codes, fmt)
    with np.errstate(all="ignore"):
        r = (d * inv).astype(np.float32)              # one float32 multiplication
    neg = ((codes & np.uint8(0x80)) != 0) & nan & ~dead
    if dtype == "float":
        q = np.where(neg, np.uint32(0xFFC00000), np.uint32(0x7FC00000)).astype(np.uint32)
        return np.where(nan | dead, q, r.view(np.uint32)).astype(np.uint32).view(np.float32)
    q = np.uint16(0x7E00 if dtype == "float16" else 0x7FC0)
    qn = np.where(neg, q | np.uint16(0x8000), q).astype(np.uint16)
    return np.where(nan | dead, qn, H.from_f32(np.where(nan | dead, np.float32(0), r), dtype)).astype(np.uint16)


def quant_multi(src, dtype, fmt):
    """src[r][k]: rank r's shard of tensor k (counts multiples of 32).  Returns
    (params8, scales8): per tensor the P shards' data bytes and scale bytes one
    after another -- bine_mx_quant_multi's two steps."""
    P, n = len(src), len(src[0])
    slots = [[quant(src[r][k], dtype, fmt) for k in range(n)] for r in range(P)]          # 1
    params8 = [np.concatenate([slots[r][k][0] for r in range(P)]) for k in range(n)]      # 2
    scales8 = [np.concatenate([slots[r][k][1] for r in range(P)]) for k in range(n)]
    return params8, scales8


# ---- inputs --------------------------------------------------------------------

def codes_of(fmt):
    """the finite non-negative values of the format, ascending"""
    if fmt == "e2m1":
        return np.array(E2M1_VALUES, dtype=np.float64)
    codes = np.arange(0x80, dtype=np.uint8)
    codes = codes[~F.is_nan8(codes, fmt) & np.isfinite(F.decode(codes, fmt))]
    return F.decode(codes, fmt).astype(np.float64)


def midpoints(fmt):
    """float32 values around every rounding boundary of the format: every
    midpoint between neighbouring codes and the float32 values one ulp either
    side, the codes themselves, values between FMAX and 2^(emax + 1), both
    signs"""
    v = codes_of(fmt)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)            # exact: one more fraction bit
    top = np.float32(FMAX[fmt])
    lim = np.float32(2.0 ** (EMAX[fmt] + 1))
    past = np.array([np.nextafter(top, np.float32(np.inf)), (top + lim) / 2, np.nextafter(lim, np.float32(0))],
                    dtype=np.float32)
    pts = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                          v.astype(np.float32), past])
    return np.concatenate([pts, -pts]).astype(np.float32)


def scale_patterns():
    """amax patterns: every binary32 exponent with fractions 0, 1 and all-ones,
    subnormals with each leading bit, zero, infinity and NaNs"""
    pats = [0, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF]
    for ex in range(1, 255):
        pats += [ex << 23, (ex << 23) | 1, (ex << 23) | 0x7FFFFF]
    for p in range(23):
        pats += [1 << p, (1 << p) | 1, (2 << p) - 1]
    return sorted(set(pats))
