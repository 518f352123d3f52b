"""The FP8 quantization contract of include/bine_amd.h restated in numpy, one
operation per line (test infrastructure).

Wide data lives on the host as float32 arrays ("float") or as uint16 bit
patterns ("float16", "bfloat16": tests/h16_util.py).  Everything here is
integer arithmetic on bit fields or a single float32 operation, so the bits
are the definition's, not a library's:

  widen_bits   the exact widening to binary32 as a map of patterns (a 16-bit
               NaN keeps sign and payload, shifted; nothing is quieted)
  amax_bits    max over the elements of widen_bits & 0x7fffffff (0 when empty)
  scale_rule   frexp / ldexp on the pattern's value
  encode       NaN -> 0x7F; clamp to +-FMAX; round to nearest even on the
               integer fields, the format's subnormals kept, -0 kept
  decode       the byte's value, exactly; a NaN byte gives the quiet NaN
               0x7fc00000 with the byte's sign
  quant / dequant / quant_multi   the entry points' statements
"""
import numpy as np

import h16_util as H

FORMATS = ("e4m3", "e5m2")
MB = {"e4m3": 3, "e5m2": 2}           # fraction bits
BIAS = {"e4m3": 7, "e5m2": 15}
FE = {"e4m3": 9, "e5m2": 16}          # FMAX = 0.875 * 2^FE
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
WIDE = ("float", "float16", "bfloat16")
NP_WIDE = {"float": np.float32, "float16": np.uint16, "bfloat16": np.uint16}


def widen_bits(x, dtype):
    """the binary32 patterns (uint32) of the elements' values"""
    if dtype == "float":
        return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b = np.ascontiguousarray(x, dtype=np.uint16).astype(np.uint32)
    if dtype == "bfloat16":
        return b << np.uint32(16)
    sign = (b & np.uint32(0x8000)) << np.uint32(16)
    ex = (b >> np.uint32(10)) & np.uint32(0x1F)
    man = b & np.uint32(0x3FF)
    # a subnormal is man * 2^-24 with its leading one at bit p
    p = np.floor(np.log2(np.maximum(man, 1))).astype(np.uint32)
    sub = ((p + np.uint32(103)) << np.uint32(23)) | ((man << (np.uint32(23) - p)) & np.uint32(0x7FFFFF))
    sub = np.where(man == 0, np.uint32(0), sub)
    norm = ((ex + np.uint32(112)) << np.uint32(23)) | (man << np.uint32(13))
    top = np.uint32(0x7F800000) | (man << np.uint32(13))
    mag = np.where(ex == 0x1F, top, np.where(ex == 0, sub, norm))
    return (sign | mag).astype(np.uint32)


def widen(x, dtype):
    return widen_bits(x, dtype).view(np.float32)


def amax_bits(x, dtype) -> int:
    w = widen_bits(x, dtype)
    return int((w & np.uint32(0x7FFFFFFF)).max()) if w.size else 0


def scale_exp(bits: int, fmt: str) -> int:
    if bits == 0 or bits >= 0x7F800000:
        return 0
    a = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    f, x = np.frexp(np.float64(a))            # a = f * 2^x, f in [0.5, 1), subnormals included
    e = FE[fmt] - int(x) - (1 if f > 0.875 else 0)
    return min(max(e, -126), 126)


def scale_rule(bits: int, fmt: str):
    """(scale, inv) as float32"""
    e = scale_exp(int(bits), fmt)
    return np.float32(np.ldexp(1.0, e)), np.float32(np.ldexp(1.0, -e))


def encode(y, fmt):
    """float32 values -> FP8 bytes"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    nan = np.isnan(y)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(y, np.float32(-FMAX[fmt])), np.float32(FMAX[fmt]))
    u = np.where(nan, np.float32(0), c).astype(np.float32).view(np.uint32).astype(np.uint64)
    mb, bias = MB[fmt], BIAS[fmt]
    sign = (u >> np.uint64(31)) << np.uint64(7)
    a = u & np.uint64(0x7FFFFFFF)
    ef = a >> np.uint64(23)
    # the format's normal range: drop 23 - mb fraction bits, nearest even, then rebase the exponent
    sh = np.uint64(23 - mb)
    lsb = (a >> sh) & np.uint64(1)
    rn = (a + ((np.uint64(1) << (sh - np.uint64(1))) - np.uint64(1)) + lsb) >> sh
    normal = rn - np.uint64((127 - bias) << mb)
    # below it: the value in units of the smallest subnormal 2^(1 - bias - mb), nearest even
    e1 = np.maximum(ef, np.uint64(1))
    sig = np.where(ef > 0, (a & np.uint64(0x7FFFFF)) | np.uint64(0x800000), a & np.uint64(0x7FFFFF))
    s = np.minimum(np.uint64(151 - bias - mb) - e1, np.uint64(40))     # value = sig * 2^(e1 - 150)
    q = sig >> s
    rem = sig & ((np.uint64(1) << s) - np.uint64(1))
    half = np.uint64(1) << (s - np.uint64(1))
    up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
    sub = q + up.astype(np.uint64)
    is_normal = ef >= np.uint64(1 - bias + 127)
    code = np.where(is_normal, normal, sub)
    return np.where(nan, np.uint64(0x7F), sign | code).astype(np.uint8)


def is_nan8(b, fmt):
    m = np.asarray(b, dtype=np.uint8) & np.uint8(0x7F)
    return m == 0x7F if fmt == "e4m3" else m > 0x7C


def decode(b, fmt):
    """FP8 bytes -> float32 values, exactly"""
    b = np.ascontiguousarray(b, dtype=np.uint8).astype(np.int64)
    mb, bias = MB[fmt], BIAS[fmt]
    mag = b & 0x7F
    ex = mag >> mb
    man = mag & ((1 << mb) - 1)
    frac = man.astype(np.float64) / (1 << mb)
    val = np.where(ex > 0, np.ldexp(1.0 + frac, ex - bias), np.ldexp(frac, 1 - bias))
    if fmt == "e5m2":
        val = np.where(mag == 0x7C, np.inf, val)
    val = np.where((b & 0x80) != 0, -val, val).astype(np.float32)
    qnan = (np.uint32(0x7FC00000) | ((b & 0x80).astype(np.uint32) << np.uint32(24))).astype(np.uint32)
    return np.where(is_nan8(b, fmt), qnan, val.view(np.uint32)).astype(np.uint32).view(np.float32)


def quant(x, dtype, fmt, scale=1.0):
    with np.errstate(all="ignore"):
        y = widen(x, dtype) * np.float32(scale)
    return encode(y, fmt)


def dequant(b, fmt, dtype, inv=1.0):
    """the destination's elements: float32 values, or uint16 patterns"""
    d = decode(b, fmt)
    nan = is_nan8(b, fmt)
    with np.errstate(all="ignore"):
        r = (d * np.float32(inv)).astype(np.float32)
    neg = (np.ascontiguousarray(b, dtype=np.uint8) & np.uint8(0x80)) != 0
    if dtype == "float":
        return np.where(nan, d.view(np.uint32), r.view(np.uint32)).astype(np.uint32).view(np.float32)
    q = np.uint16(0x7E00 if dtype == "float16" else 0x7FC0)
    qn = np.where(neg, q | np.uint16(0x8000), q).astype(np.uint16)
    return np.where(nan, qn, H.from_f32(np.where(nan, np.float32(0), r), dtype)).astype(np.uint16)


def quant_multi(src, dtype, fmt):
    """src[r][k]: rank r's shard of tensor k.  Returns (params8, scales):
    params8[k] = the P shards' bytes one after another, scales = 2n float32 --
    bine_quant_multi's five steps."""
    P, n = len(src), len(src[0])
    amax = [[amax_bits(src[r][k], dtype) for k in range(n)] for r in range(P)]           # 1
    agreed = [max(amax[r][k] for r in range(P)) for k in range(n)]                       # 2
    rules = [scale_rule(agreed[k], fmt) for k in range(n)]                               # 3
    scales = np.array([s for s, _ in rules] + [i for _, i in rules], dtype=np.float32)
    slots = [[quant(src[r][k], dtype, fmt, scales[k]) for k in range(n)] for r in range(P)]   # 4
    params8 = [np.concatenate([slots[r][k] for r in range(P)]) for k in range(n)]        # 5
    return params8, scales


# ---- inputs --------------------------------------------------------------------

def all16(dtype):
    """all 65,536 patterns of a 16-bit type"""
    assert dtype in H.TYPES
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def midpoints(fmt):
    """float32 values around every rounding boundary of the format: for each
    finite code the midpoint to its neighbour of larger magnitude and the
    float32 values one ulp either side of it, both signs; then values at and
    past FMAX (the clamp), the infinities and zeros"""
    codes = np.arange(0x80, dtype=np.uint8)
    codes = codes[~is_nan8(codes, fmt) & np.isfinite(decode(codes, fmt))]
    v = decode(codes, fmt).astype(np.float64)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)            # exact: one more fraction bit
    pts = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                          v.astype(np.float32)])
    top = np.float32(FMAX[fmt])
    past = np.array([np.nextafter(top, np.float32(np.inf)), top * np.float32(1.03125), top * np.float32(1.0625),
                     top * np.float32(2), 3.0e38, np.finfo(np.float32).max, np.inf, 1e-45, 1e-39], dtype=np.float32)
    pts = np.concatenate([pts, past])
    return np.concatenate([pts, -pts]).astype(np.float32)


def boundary_patterns(fmt):
    """amax patterns around every decision of the scale rule"""
    f32 = lambda v: int(np.array([v], dtype=np.float32).view(np.uint32)[0])  # noqa: E731
    top = f32(FMAX[fmt])
    pats = [0, 1, 2, 3, 0x007FFFFF, 0x00800000, top - 1, top, top + 1, 0x7F7FFFFF, 0x7F800000, 0x7FC00000,
            0x7F800001, 0x7FFFFFFF]
    for ex in range(1, 255):                     # every normal power of two; 0.875 * 2^x and its neighbours
        pats += [ex << 23, (ex << 23) | 0x600000, ((ex << 23) | 0x600000) - 1, ((ex << 23) | 0x600000) + 1]
    for p in range(23):                          # the subnormal powers of two and 0.875 * 2^x among them
        pats.append(1 << p)
        if p >= 3:
            seven = 7 << (p - 2)                 # 1.75 * 2^p in units of 2^-149
            pats += [seven, seven - 1, seven + 1]
    return sorted(set(pats))
