"""The MX-quantized gradient reduce-scatter of include/bine_amd.h restated in
numpy, one operation per line (test infrastructure): the wire layout of a
bucket, the pack step, the exchange and the ordered float32 sum.  Quantization
and decoding are tests/mx_sim.py's.

  layout        (data offsets, scale offsets, D, B) of a bucket
  pack_block    one contribution: the shards of the n tensors -> B bytes
  values        a block's elements as float32 (decode * 2^(S - 127), exact),
                their scale bytes one per element
  sum_blocks    dst of bine_mx_sum_segments, and where its bits are specified
  reduce_scatter   pack + exchange + sum over P ranks
"""
import numpy as np

import h16_util as H
import mx_sim as M

QNAN = {"float": 0x7FC00000, "float16": 0x7E00, "bfloat16": 0x7FC0}
VIEW = {"float": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}
# the larger of the top binade's half-spacing and the clamp gap 2^(emax + 1) - FMAX, in units of 2^(S - 127)
E_FMT = {"e4m3": 64.0, "e5m2": 8192.0, "e2m1": 2.0}


def layout(counts, fmt):
    assert all(c % M.BLOCK == 0 for c in counts)
    doff, soff, d, s = [], [], 0, 0
    for c in counts:
        doff.append(d)
        soff.append(s)
        d += M.dbytes(c, fmt)
        s += c // M.BLOCK
    B = (d + s + 15) // 16 * 16
    return doff, [d + o for o in soff], d, B


def pack_block(shards, dtype, fmt, pad=0):
    """the wire block of one contribution: shards[k] = tensor k's elements"""
    counts = [x.size for x in shards]
    doff, soff, _, B = layout(counts, fmt)
    blk = np.full(B, pad, dtype=np.uint8)
    for k, x in enumerate(shards):
        q, s = M.quant(x, dtype, fmt)
        blk[doff[k]:doff[k] + q.size] = q
        blk[soff[k]:soff[k] + s.size] = s
    return blk


def values(blk, counts, fmt):
    """per tensor (d, S): the float32 value of every element -- a quiet NaN for
    a NaN data byte and under S = 0xFF -- and its block's scale byte"""
    doff, soff, _, _ = layout(counts, fmt)
    out = []
    for k, c in enumerate(counts):
        data = blk[doff[k]:doff[k] + M.dbytes(c, fmt)]
        S = blk[soff[k]:soff[k] + c // M.BLOCK]
        out.append((M.dequant(data, S, c, fmt, "float"), np.repeat(S, M.BLOCK)))
    return out


def sum_blocks(blocks, counts, fmt, ddtype, scale=1.0):
    """per tensor (bits, exact): dst's patterns, and a mask of the elements whose
    bits the contract fixes -- everything but a NaN that arithmetic made (from a
    NaN or infinity data byte), whose payload is open"""
    per = [values(b, counts, fmt) for b in blocks]
    out = []
    for k, c in enumerate(counts):
        acc = per[0][k][0].copy()
        dead = per[0][k][1] == 0xFF
        with np.errstate(all="ignore"):
            for j in range(1, len(blocks)):
                acc = (acc + per[j][k][0]).astype(np.float32)          # one float32 addition, in stream order
                dead |= per[j][k][1] == 0xFF
            r = (acc * np.float32(scale)).astype(np.float32)           # one float32 multiplication
        if ddtype == "float":
            bits = r.view(np.uint32).copy()
        else:
            bits = H.from_f32(np.where(np.isnan(r), np.float32(0), r), ddtype)     # one rounding, nearest even
        bits = np.where(dead, VIEW[ddtype](QNAN[ddtype]), bits).astype(VIEW[ddtype])
        out.append((bits, dead | ~np.isnan(r)))
    return out


def is_nan(bits, ddtype):
    bits = np.asarray(bits)
    if ddtype == "float":
        return (bits & 0x7FFFFFFF) > 0x7F800000
    inf = 0x7C00 if ddtype == "float16" else 0x7F80
    return (bits & 0x7FFF) > inf


def same(got, want, ddtype):
    """got against sum_blocks' (bits, exact): equal where exact, some NaN elsewhere; the first bad indices"""
    bits, exact = want
    ok = np.where(exact, got == bits, is_nan(got, ddtype))
    return np.nonzero(~ok)[0][:4]


def reduce_scatter(src, counts, sdtype, rdtype, fmt, scale=1.0):
    """src[r][k]: rank r's tensor k, P shards of counts[k] elements one after
    another.  Returns (rbufs[r][k] as sum_blocks gives them, recv[r]: the P
    blocks rank r received, block j from rank j)"""
    P = len(src)
    send = [[pack_block([src[r][k][j * c:(j + 1) * c] for k, c in enumerate(counts)], sdtype, fmt) for j in range(P)]
            for r in range(P)]                                                                     # 1
    recv = [[send[j][r] for j in range(P)] for r in range(P)]                                       # 2
    return [sum_blocks(recv[r], counts, fmt, rdtype, scale) for r in range(P)], recv               # 3
