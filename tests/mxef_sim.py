"""MX quantization with an error-feedback residual (bine_mx_quant_ef_segments,
bine_mx_reduce_scatter_multi_ef; include/bine_amd.h) restated in numpy, one
operation per line (test infrastructure).  Quantization and decoding are
tests/mx_sim.py's, the wire layout and the ordered sum tests/mxrs_sim.py's.

  quant_ef           (data bytes, scale bytes, new residual) of one segment
  reduce_scatter_ef  pack with quant_ef + exchange + sum over P ranks; the
                     ranks' new residuals beside the shards
"""
import numpy as np

import fp8_sim as F
import mx_sim as M
import mxrs_sim as R

E_FMT = R.E_FMT


def add(x, r, dtype):
    """v = widen(x) + r: one float32 addition"""
    with np.errstate(all="ignore"):
        return (F.widen(x, dtype) + np.ascontiguousarray(r, dtype=np.float32)).astype(np.float32)


def quant_ef(x, r, dtype, fmt):
    """x: the source's elements (float32, or uint16 patterns), r: float32.
    Returns (data, S, r'): M.quant's bytes for v = widen(x) + r as a float
    source, and r' = v - decode * 2^(S - 127), +0.0 in a block with S = 0xFF."""
    v = add(x, r, dtype)
    data, S = M.quant(v, "float", fmt)                    # A and S over the block's v; the codes of v under S
    d = M.dequant(data, S, v.size, fmt, "float")          # one float32 multiplication, exact
    dead = np.repeat(S, M.BLOCK)[:v.size] == 0xFF
    with np.errstate(all="ignore"):
        rn = (v - np.where(dead, np.float32(0), d)).astype(np.float32)     # one float32 subtraction
    return data, S, np.where(dead, np.float32(0), rn).astype(np.float32)


def pack_block_ef(shards, res, dtype, fmt, pad=0):
    """the wire block of one contribution and the shards' new residuals"""
    counts = [x.size for x in shards]
    doff, soff, _, B = R.layout(counts, fmt)
    blk = np.full(B, pad, dtype=np.uint8)
    out = []
    for k, (x, r) in enumerate(zip(shards, res)):
        q, s, rn = quant_ef(x, r, dtype, fmt)
        blk[doff[k]:doff[k] + q.size] = q
        blk[soff[k]:soff[k] + s.size] = s
        out.append(rn)
    return blk, out


def reduce_scatter_ef(src, res, counts, sdtype, rdtype, fmt, scale=1.0):
    """src[r][k], res[r][k]: rank r's tensor k and its residual, P shards of
    counts[k] elements one after another.  Returns (rbufs[r][k] as
    mxrs_sim.sum_blocks gives them, res'[r][k], recv[r])."""
    P = len(src)
    send, new = [], []
    for r in range(P):
        packed = [pack_block_ef([src[r][k][j * c:(j + 1) * c] for k, c in enumerate(counts)],
                                [res[r][k][j * c:(j + 1) * c] for k, c in enumerate(counts)], sdtype, fmt)
                  for j in range(P)]                                                                    # 1
        send.append([p[0] for p in packed])
        new.append([np.concatenate([packed[j][1][k] for j in range(P)]) if c else np.zeros(0, dtype=np.float32)
                    for k, c in enumerate(counts)])
    recv = [[send[j][r] for j in range(P)] for r in range(P)]                                          # 2
    return [R.sum_blocks(recv[r], counts, fmt, rdtype, scale) for r in range(P)], new, recv             # 3
