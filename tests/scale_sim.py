"""Host replay of SCALED issue schedules, and the host form of S (test
infrastructure).

tests/plan_sim.py replays the unscaled plans; it knows neither the
BINE_PRIM_SCALED flag of a REDUCE_TREE nor the SCALE primitive.  run() below
restates its replay for the schedules `pico_amd.schedule(..., scaled=...)`
returns -- the same rendezvous rules: the sends and receives of one exchange
op are posted together, a transfer happens when the head send and the head
receive of a (src, dst) pair are both posted and carry the same count, a rank
posts its next op only after the current one completed, no progress =
deadlock -- and applies `scale` where the schedule says so: to the output of a
flagged tree, and to the range of a SCALE primitive.

S() is include/bine_amd.h's definition on the host: float / double multiply in
their own format by float32(scale) / scale; the 16-bit types (uint16 bit
patterns, tests/h16_util.py) are widened exactly to float32, multiplied by
float32(scale) in float32 and rounded to nearest even into the 16-bit format.
"""
import collections

import numpy as np

import h16_util as H
import pico_amd
from oracle import oracle as O
from pico_amd._lib import PRIM_SCALED

SB, RB = 0, 1


class SimError(AssertionError):
    pass


def S(x, dtype, scale):
    with np.errstate(all="ignore"):
        if dtype in H.TYPES:
            return H.from_f32(H.to_f32(x, dtype) * np.float32(scale), dtype)
        if dtype == "float":
            return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)
        assert dtype == "double"
        return np.asarray(x, np.float64) * np.float64(scale)


def reduce_local(inp, inout, dtype, op):
    (H.reduce_local if dtype in H.TYPES else O.reduce_local)(inp, inout, dtype, op)


def np_dtype(dtype):
    return np.uint16 if dtype in H.TYPES else O.NP_DTYPES[dtype]


def schedules(coll, algo, P, esz, count=0, rcounts=None, in_place=False, chunk_bytes=0, flat_ag=False,
              flat_rs=False, scaled=False, trees=False):
    """[(ops, info)] per rank"""
    out = []
    for r in range(P):
        ops, _, _, info = pico_amd.schedule(coll, algo, P, r, count=count, rcounts=rcounts, esz=esz,
                                            in_place=in_place, chunk_bytes=chunk_bytes, info=True, trees=trees,
                                            flat_ag=flat_ag, flat_rs=flat_rs, scaled=scaled)
        out.append((ops, info))
    return out


def strip(ops):
    """a scaled schedule with the SCALED flag cleared and the SCALE primitives
    (and the ops they leave empty) removed"""
    out = []
    for o in ops:
        prims = []
        for p in o["prims"]:
            if p["type"] == "SCALE":
                continue
            q = dict(p)
            if q["type"] == "REDUCE_TREE":
                q["flags"] &= ~PRIM_SCALED
            prims.append(q)
        if prims:
            out.append({"xchg": o["xchg"], "wait": o["wait"], "prims": prims})
    return out


def run(coll, algo, sbufs, dtype, op="sum", rcounts=None, in_place=False, chunk_bytes=0, flat_ag=False,
        flat_rs=False, scale=None, trees=False, counter=None):
    """Replay all ranks' issue schedules (scaled when `scale` is given) on
    copies of `sbufs`; returns the output of every rank.  `counter` (a
    collections.Counter) receives how many flagged trees and SCALE primitives
    ran."""
    P = len(sbufs)
    nd = np_dtype(dtype)
    count = sbufs[0].size
    sch = schedules(coll, algo, P, np.dtype(nd).itemsize, count=count, rcounts=rcounts, in_place=in_place,
                    chunk_bytes=chunk_bytes, flat_ag=flat_ag, flat_rs=flat_rs, scaled=scale is not None,
                    trees=trees)
    bufs = []
    for r in range(P):
        nout = max(rcounts[r] if coll == "reduce_scatter" else count, 1)
        if in_place:
            rb = np.array(sbufs[r], dtype=nd).copy()
            sb = rb
        else:
            sb = np.array(sbufs[r], dtype=nd).copy()
            rb = np.full(nout, 0xA5A5 if nd == np.uint16 else np.nan, dtype=nd)
        info = sch[r][1]
        tb = [np.full(int(t) + 16, 0xA5A5 if nd == np.uint16 else np.nan, dtype=nd)
              for t in info["tmp_elems"] + [info["stage_elems"]]]
        bufs.append([sb, rb] + tb)

    def view(r, buf, off, n):
        b = bufs[r][buf]
        if off + n > b.size:
            raise SimError(f"rank {r}: buffer {buf} overflow ({off}+{n} > {b.size})")
        return b[off:off + n]

    def local(r, p):
        n = p["count"]
        if p["type"] == "COPY":
            view(r, p["dst_buf"], p["dst_off"], n)[:] = view(r, p["src_buf"], p["src_off"], n).copy()
        elif p["type"] == "SCALE":
            if scale is None:
                raise SimError("SCALE in an unscaled schedule")
            view(r, p["dst_buf"], p["dst_off"], n)[:] = S(view(r, p["src_buf"], p["src_off"], n).copy(), dtype, scale)
            if counter is not None:
                counter["scale"] += 1
        elif p["type"] == "REDUCE":
            io = view(r, p["dst_buf"], p["dst_off"], n)
            t = io.copy()
            reduce_local(np.ascontiguousarray(view(r, p["src_buf"], p["src_off"], n)), t, dtype, op)
            io[:] = t
        elif p["type"] == "REDUCE3":
            b = view(r, p["aux_buf"], p["aux_off"], n).copy()
            reduce_local(np.ascontiguousarray(view(r, p["src_buf"], p["src_off"], n)), b, dtype, op)
            view(r, p["dst_buf"], p["dst_off"], n)[:] = b
        elif p["type"] == "REDUCE_TREE":
            nl, pos = p["peer"], p["pos"]
            others = iter(range(nl - 1))
            v = [view(r, p["aux_buf"], p["aux_off"], n).copy() if j == pos else
                 view(r, p["src_buf"], p["src_off"] + next(others) * n, n).copy() for j in range(nl)]
            w, lvl, swap = 1, 0, p["flags"] >> 8
            while w < nl:
                for i in range(0, nl, 2 * w):
                    if (swap >> lvl) & 1:
                        t = v[i + w].copy()
                        reduce_local(np.ascontiguousarray(v[i]), t, dtype, op)
                        v[i] = t
                    else:
                        reduce_local(np.ascontiguousarray(v[i + w]), v[i], dtype, op)
                w *= 2
                lvl += 1
            res = v[0]
            if p["flags"] & PRIM_SCALED:
                if scale is None:
                    raise SimError("flagged tree in an unscaled schedule")
                res = S(res, dtype, scale)
                if counter is not None:
                    counter["tree"] += 1
            view(r, p["dst_buf"], p["dst_off"], n)[:] = res
        else:
            raise SimError(f"unknown local primitive {p['type']}")

    pc = [0] * P
    posted = [False] * P
    pending = [0] * P
    sendq, recvq = collections.defaultdict(collections.deque), collections.defaultdict(collections.deque)
    while True:
        progress = False
        for r in range(P):
            ops = sch[r][0]
            while pc[r] < len(ops) and not posted[r]:
                o = ops[pc[r]]
                if not o["xchg"]:
                    for p in o["prims"]:
                        local(r, p)
                    pc[r] += 1
                else:
                    for p in o["prims"]:
                        (sendq[(r, p["peer"])] if p["type"] == "SEND" else recvq[(p["peer"], r)]).append((r, p))
                    posted[r], pending[r] = True, len(o["prims"])
                progress = True
        for key in list(sendq):
            while sendq[key] and recvq[key]:
                (sr, s), (rr, rv) = sendq[key].popleft(), recvq[key].popleft()
                if s["count"] != rv["count"]:
                    raise SimError(f"{key}: send {s['count']} vs recv {rv['count']}")
                view(rr, rv["dst_buf"], rv["dst_off"], rv["count"])[:] = \
                    view(sr, s["src_buf"], s["src_off"], s["count"]).copy()
                pending[sr] -= 1
                pending[rr] -= 1
                progress = True
        for r in range(P):
            if posted[r] and pending[r] == 0:
                posted[r] = False
                pc[r] += 1
                progress = True
        if all(pc[r] >= len(sch[r][0]) and not posted[r] for r in range(P)):
            break
        if not progress:
            raise SimError(f"deadlock: pcs={pc}")
    return [bufs[r][RB][:(rcounts[r] if coll == "reduce_scatter" else count)] for r in range(P)]
