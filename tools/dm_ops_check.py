#!/usr/bin/env python3
"""The direct peer-memory transport's own reductions -- k_dm_fused<T, OP>
(dmf::tree_slice) and k_dm_move_tree<T, OP, NL> (tree_tile on the inbox slots)
-- on every element type and op they are instantiated for (float, double,
int32, uint32, int64, uint64 x SUM, PROD, MAX, MIN), at the vector counts
where their slice and tile arithmetic can go wrong, with inputs that tell the
24 (type, op) pairs apart: P processes share the box's GPU, every rank's
output is compared byte for byte with the oracle, the bytes past each output's
end must stay untouched, and every row asserts the FORM its call took
(bine_comm_fused_calls and the kinds of the BINE_DIRECT_STAMPS records: 4 =
k_dm_fused, 2 = a tree inside k_dm_move_tree, 0 / 1 = k_dm_move copies):

  small     one k_dm_fused launch of a single-stream call (d.wgs workgroups)
  large     the same shapes with BINE_SINGLE_STREAM_BYTES=0: fused_for, counted
  tree      allreduces the one-launch form refuses (chunks below one slot, or
            the literal allgather): the trees hosted by exchange launches,
            deferred into the next exchange, in their own exchange, or -- the
            last chunk's -- in a launch of their own
  rs        reduce_scatter bine_permute_remap of 1, 4 and 6 chunks: one
            launch, a full launch, two launches
  fallback  blocks that are no multiple of 16 B on any rank, fused trees off
            (set_direct_tree(0)), P = 3: k_dm_move copies and separate
            reduction kernels, never an in-launch form

MODE small runs in the default environment, MODE large with
BINE_SINGLE_STREAM_BYTES=0 (no call is single-stream) and
BINE_DIRECT_TREE_WGS=1, so that set_direct_tree(1) means ONE tree workgroup
(set_direct_tree(n > 1) sets n; 256 is the library's default count).  Both
use 1 MiB slots.  Consecutive rows reuse each ordered pair's four slots with
the same vector count, with another one (the kGeomOff record) and with
one-launch and per-exchange calls interleaved; rows with wgs = MIXED give
every rank its own set_direct_wgs (the slice flags carry the cut).

cases(P, mode) is the table (importable without torch or a GPU;
tests/test_dm_ops_cases.py proves on the CPU that every row reaches the form
it names and can tell a wrong dispatch from the right one).
usage: python tools/dm_ops_check.py P MODE   (exit 0 = every rank, every row ok)
"""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOT = 1 << 20
GUARD = 256        # bytes past every output's end that must stay untouched
MIXED = -1         # wgs: every rank its own count (rank + 1)
TYPES = (("float", 4), ("double", 8), ("int32", 4), ("uint32", 4), ("int64", 8), ("uint64", 8))
OPS = ("sum", "prod", "max", "min")
PAIRS = tuple((dt, op) for dt, _ in TYPES for op in OPS)
ESZ = dict(TYPES)
VS = (1, 3, 255, 256, 257, 1025)   # 16-byte vectors per rank's block
FULL = (("float", "sum"), ("uint64", "max"), ("int32", "min"))   # pairs that run every v
WGS = (0, 1, 3)            # set_direct_wgs: default, 1, 3
TREE_WGS = (256, 1, 3)     # set_direct_tree: the default count, 1 (large mode's environment), 3
FORMS = ("small", "large", "tree", "rs", "fallback")
MODES = ("small", "large")

Row = collections.namedtuple("Row", "coll algo dtype op n inplace chunk flat_ag wgs tree form")
Row.__doc__ = """n: elements per rank (allreduce) or per block (reduce_scatter); chunk: the pipelining
chunk in bytes (0 = the default, unchunked here); flat_ag: set_flat_ag's value; wgs: set_direct_wgs's (MIXED:
rank + 1); tree: set_direct_tree's; form: the form the call must take"""


def _vs(k, pair):
    return VS if pair in FULL else (VS[k % len(VS)],)


def _fused_rows(P, form):
    """unchunked flat allreduces with blocks of v vectors: one k_dm_fused launch"""
    out = []
    for k, (dt, op) in enumerate(PAIRS):
        for i, v in enumerate(_vs(k, (dt, op))):
            algo = "bine_bdw_static" if (k + i) % 4 == 3 else "bine_bdw_remap"
            out.append(Row("allreduce", algo, dt, op, P * v * 16 // ESZ[dt], (k + i) % 3 == 1, 0, 2,
                           WGS[(k + i) % 3], TREE_WGS[(k + i + 1) % 3] if form == "large" else 1, form))
    return out


def _tree_rows(P):
    """allreduces the one-launch form refuses, their trees hosted by exchange launches: 2 or 3 chunks
    of v vectors per block (below one slot) with the flat allgather -- every tree but the last deferred
    into the next chunk's exchange, the last in a launch of its own (flat_ag 1) or deferred into the
    allgather's piece (flat_ag 2) -- and one chunk followed by the literal allgather (flat_ag 0): the
    tree inside its own exchange"""
    out = []
    for k, (dt, op) in enumerate(PAIRS):
        for i, v in enumerate(_vs(k + 2, (dt, op))):
            flat_ag = (1, 2, 0 if P > 2 else 1)[(k + i) % 3]   # (P = 2: the literal allgather IS the flat one)
            nch = 2 + (k + i) // 3 % 2 if flat_ag else 1
            out.append(Row("allreduce", "bine_bdw_remap", dt, op, P * v * nch * 16 // ESZ[dt], (k + i) % 4 == 2,
                           v * 16 if flat_ag else 0, flat_ag, WGS[(k + i + 1) % 3], TREE_WGS[(k + i) % 3], "tree"))
    return out


def _reuse_rows(P, form):
    """the head of the table: each ordered pair's four slots reused by one-launch calls of the same
    vector count (two slots per call at P = 2), then of another count, then with per-exchange calls
    (odd counts) between them"""
    def ar(dt, op, v, odd=0):
        return Row("allreduce", "bine_bdw_remap", dt, op, P * (v * 16 // ESZ[dt] + odd), False, 0, 2, 0, 1,
                   "fallback" if odd else form)
    same = [ar("float", "sum", 257), ar("int32", "min", 257), ar("uint64", "max", 257), ar("double", "prod", 257),
            ar("uint32", "max", 257)]
    other = [ar("float", "sum", 3), ar("int64", "min", 3), ar("float", "sum", 1025), ar("double", "max", 1)]
    mixed = [ar("float", "sum", 257, 1), ar("float", "sum", 257), ar("int32", "sum", 3, 1), ar("uint64", "max", 257),
             ar("float", "max", 255, 1), ar("float", "sum", 257)]
    return same + other + mixed


def _rs_rows(P):
    out = []
    for k, (dt, op) in enumerate(PAIRS):
        for i, nch in enumerate((1, 4, 6) if (dt, op) in FULL else ((1, 4, 6)[k % 3],)):
            v = VS[(k + i + 4) % len(VS)]
            out.append(Row("reduce_scatter", "bine_permute_remap", dt, op, v * nch * 16 // ESZ[dt], False,
                           v * 16, 2, WGS[(k + i) % 3], TREE_WGS[(k + i + 2) % 3], "rs"))
    return out


def _fallback_rows(P, mode):
    """blocks of v vectors and one element (no multiple of 16 B on any rank) in both modes; in large
    mode also aligned shapes with the fused trees off"""
    out = []
    for k, (dt, op) in enumerate(PAIRS):
        if k % 3 != (0 if mode == "small" else 1):
            continue
        v = VS[(k // 3) % len(VS)]
        out.append(Row("allreduce", "bine_bdw_remap", dt, op, P * (v * 16 // ESZ[dt] + 1), k % 2 == 0, 0, 2,
                       WGS[k % 3], 1, "fallback"))
        if mode == "large":
            out.append(Row("allreduce", "bine_bdw_remap", dt, op, P * v * 2 * 16 // ESZ[dt], False, v * 16, 2,
                           WGS[(k + 1) % 3], 0, "fallback"))
            out.append(Row("reduce_scatter", "bine_permute_remap", dt, op, v * 16 // ESZ[dt] + 1, False, 0, 2,
                           WGS[(k + 2) % 3], 1, "fallback"))
    return out


def _mixed_rows(P, mode):
    """every rank cuts its messages with its own workgroup count"""
    out = []
    for i, v in enumerate(VS):
        n = P * v * 4
        if mode == "small":
            out.append(Row("allreduce", "bine_bdw_remap", "float", "sum", n, i % 2 == 1, 0, 2, MIXED, 1, "small"))
        else:
            out.append(Row("allreduce", "bine_bdw_remap", "float", "sum", 2 * n, False, v * 16, 2, MIXED,
                           TREE_WGS[i % 3], "tree"))
    if mode == "large":
        out.append(Row("allreduce", "bine_bdw_remap", "float", "sum", P * 257 * 4, False, 0, 2, MIXED, 3, "large"))
        out.append(Row("allreduce", "bine_bdw_remap", "uint64", "max", P * (3 * 2 + 1), False, 0, 2, MIXED, 1, "fallback"))
    return out


def _p3_rows():
    """P = 3: no flat trees (they need a power-of-two P), the literal schedules' k_dm_move traffic"""
    algos = (("allreduce", "ring"), ("allreduce", "rabenseifner"), ("allreduce", "bine_lat"), ("reduce_scatter", "ring"))
    out = []
    for k, (dt, op) in enumerate(PAIRS):
        coll, algo = algos[(k + k // 4) % 4]
        v = VS[k % len(VS)]
        n = 3 * v * 16 // ESZ[dt] + (k // 4) % 2   # even and odd counts
        if coll == "reduce_scatter":
            n = v * 16 // ESZ[dt] + (k // 4) % 2
        out.append(Row(coll, algo, dt, op, n, k % 5 == 2, 0 if k % 2 else 4096, 0, WGS[k % 3], 1, "fallback"))
    return out


def _interleave(groups):
    """round-robin over the groups: the forms alternate on every pair's slots, and rows of one
    group that follow each other keep (FULL pairs: change) the vector count"""
    out, its = [], [list(g) for g in groups if g]
    while its:
        for g in list(its):
            out.append(g.pop(0))
            if not g:
                its.remove(g)
    return out


def _first_per_pair(rows):
    seen, out = set(), []
    for r in rows:
        if (r.dtype, r.op) not in seen:
            seen.add((r.dtype, r.op))
            out.append(r)
    return out


def cases(P, mode):
    """the rows P ranks run in MODE, in call order"""
    assert mode in MODES, mode
    if P == 3:
        return _p3_rows() if mode == "large" else []
    if P == 8:   # the reduced table: every pair once as one launch, once with hosted trees (NL = 8)
        assert mode == "large"
        return _interleave([_first_per_pair(_fused_rows(P, "large")), _first_per_pair(_tree_rows(P))])
    if mode == "small":
        return _reuse_rows(P, "small") + _interleave([_fused_rows(P, "small"), _fallback_rows(P, mode),
                                                      _mixed_rows(P, mode)])
    return _reuse_rows(P, "large") + _interleave([_fused_rows(P, "large"), _tree_rows(P), _rs_rows(P),
                                                  _fallback_rows(P, mode), _mixed_rows(P, mode)])


def environment(mode):
    """what the workers set before the communicator exists"""
    env = {"BINE_DIRECT_SLOT_BYTES": str(SLOT), "BINE_DIRECT_STAMPS": str(1 << 16)}
    if mode == "large":
        env.update(BINE_SINGLE_STREAM_BYTES="0", BINE_DIRECT_TREE_WGS="1")
    return env


def total_count(row, P):
    return row.n if row.coll == "allreduce" else row.n * P


def inputs(row, P, seed):
    """the oracle's generator, then planted values that tell the (type, op) pairs apart; element i of
    rank r, k = i % 8, g = i // 8:
      float / double  k = 1: one rank holds NaN (one encoding), +inf or -inf; k = 2: signed zeros, the
                      sign alternating over the ranks; k = 3: denormals of both signs; k >= 4 of the
                      first 16 elements: zeros, each rank in turn the only negative one (MAX / MIN
                      keep one operand of a tie: which one shows the operand order)
      signed          k = 1: negated on alternating ranks; k = 2: the type's min on one rank and its
                      max on the next; k = 3: -1 on alternating ranks
      unsigned        k = 1: the top bit set on alternating ranks; k = 2: the top bit set on every
                      rank; k = 3: the type's max on one rank
    PROD: the other elements have magnitudes near 1 (floats 0.75 .. 1.25 of either sign, integers
    1 .. 4), so that the product of 8 ranks neither overflows nor collapses to 0."""
    import numpy as np
    from oracle import oracle as O
    n = total_count(row, P)
    dt, op = row.dtype, row.op
    np_dt = np.dtype(O.NP_DTYPES[dt])
    sb = O.inputs(dt, n, P, seed_base=seed)
    i = np.arange(n)
    k, g = i % 8, i // 8
    for r in range(P):
        x = sb[r]
        alt = (r + g) % 2 == 0
        one = (g + i) % P == r
        nxt = (g + i + 1) % P == r
        if np_dt.kind == "f":
            if op == "prod":
                x[:] = (0.75 + x / 200) * np.where((i + r) % 3 == 0, -1, 1)
            fi = np.finfo(np_dt)
            x[(k == 1) & one] = np.array([np.nan, np.inf, -np.inf], np_dt)[g % 3][(k == 1) & one]
            x[k == 2] = np.where(alt, -0.0, 0.0)[k == 2]
            tiny = (fi.smallest_subnormal * (1 + r + i % 7) * np.where(alt, 1, -1)).astype(np_dt)
            x[k == 3] = tiny[k == 3]
            sole = (k >= 4) & (g < 2)
            x[sole] = np.where((k - 4 + 4 * g) % P == r, -0.0, 0.0)[sole]
        elif np_dt.kind == "i":
            ii = np.iinfo(np_dt)
            if op == "prod":
                x[:] = (x % 4 + 1) * np.where((i + r) % 3 == 0, -1, 1)
            x[(k == 1) & alt] = -x[(k == 1) & alt]
            x[(k == 2) & one] = ii.min
            x[(k == 2) & nxt & ~one] = ii.max
            x[(k == 3) & alt] = -1
        else:
            ii = np.iinfo(np_dt)
            top = np_dt.type(1) << np_dt.type(8 * np_dt.itemsize - 1)
            if op == "prod":
                x[:] = x % np_dt.type(4) + np_dt.type(1)
            x[(k == 1) & alt] |= top
            x[k == 2] |= top
            x[(k == 3) & one] = ii.max
    return sb


def planted(n):
    """mask of the positions inputs() plants"""
    import numpy as np
    k, g = np.arange(n) % 8, np.arange(n) // 8
    return ((k >= 1) & (k <= 3)) | ((k >= 4) & (g < 2))


def expected(row, P, sb):
    """every rank's output by the oracle (the literal schedule's bits)"""
    from oracle import oracle as O
    if row.coll == "allreduce":
        want, rets = O.allreduce(row.algo, sb, row.dtype, row.op)
    else:
        want, rets = O.reduce_scatter(row.algo, sb, [row.n] * P, row.dtype, row.op)
    assert not any(rets), (row, rets)
    return want


def seed_of(index):
    return 1234 + 16 * index


def launches_of(row):
    """k_dm_fused launches of an rs row: one per 4 chunks"""
    nch = -(-row.n * ESZ[row.dtype] // row.chunk) if row.chunk else 1
    return -(-nch // 4)


def check_form(row, took, stamps):
    """'' or what is wrong with the form the call took: `took` = the delta of fused_calls(),
    stamps = the call's BINE_DIRECT_STAMPS records"""
    kinds = sorted({int(t) >> 24 & 0xff for t in stamps[:, 0]})
    fused_serials = len({int(t) >> 32 for t in stamps[:, 0] if int(t) >> 24 & 0xff == 4})
    what = f"fused_calls +{took}, stamp kinds {kinds}, {fused_serials} k_dm_fused launches"
    if row.form == "small":
        ok = took == 0 and kinds == [4] and fused_serials == 1
    elif row.form == "large":
        ok = took == 1 and kinds == [4] and fused_serials == 1
    elif row.form == "rs":
        ok = took == 1 and kinds == [4] and fused_serials == launches_of(row)
    elif row.form == "tree":
        ok = took == 0 and 2 in kinds and 4 not in kinds
    else:
        ok = took == 0 and 2 not in kinds and 4 not in kinds and len(kinds) > 0
    return "" if ok else f"form {row.form} not taken: {what}"


def worker(rank, P, mode, port, q):
    from tools._procs import rank_device
    dev = rank_device(rank)   # (sets the fake RCCL host id on the one-GPU box)
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")
    os.environ.update(environment(mode))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    import numpy as np
    import pico_amd
    import torch
    import torch.distributed as dist
    from oracle import oracle as O
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    comm.set_direct(True)
    comm.set_flat_rs(True)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    comm.direct_stamps()   # (reset)
    for index, row in enumerate(cases(P, mode)):
        np_dt = np.dtype(O.NP_DTYPES[row.dtype])
        esz = np_dt.itemsize
        sb = inputs(row, P, seed_of(index))
        want = np.ascontiguousarray(expected(row, P, sb)[rank])
        total = total_count(row, P)
        outn = row.n
        comm.set_flat_ag(row.flat_ag)
        comm.set_chunk(row.chunk)
        comm.set_direct_wgs(rank + 1 if row.wgs == MIXED else row.wgs)
        comm.set_direct_tree(row.tree)
        s = torch.from_numpy(sb[rank].view(np.uint8).copy()).to("cuda")
        r = torch.full(((total if row.inplace else outn) * esz + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        if row.inplace:
            r[:total * esz] = s
        torch.cuda.synchronize()
        before = comm.fused_calls()
        tag = " ".join(str(x) for x in (index,) + tuple(row))
        try:
            with torch.cuda.stream(side):
                src = pico_amd.IN_PLACE if row.inplace else s
                if row.coll == "allreduce":
                    pico_amd.allreduce(row.algo, src, r, row.n, row.dtype, row.op, comm)
                else:
                    pico_amd.reduce_scatter(row.algo, src, r, [row.n] * P, row.dtype, row.op, comm)
            torch.cuda.synchronize()
            comm.synchronize()
        except Exception as e:  # noqa: BLE001 -- a row that errors fails; the peers may be waiting: stop here
            print(f"rank {rank} MISMATCH {tag}: {type(e).__name__}: {e}", flush=True)
            raise
        host = r.cpu().numpy()
        got = host[:outn * esz]
        tail = host[(total if row.inplace else outn) * esz:]
        took = comm.fused_calls() - before
        why = check_form(row, took, comm.direct_stamps())
        diff = np.flatnonzero(got != want.view(np.uint8))
        if diff.size:
            why = f"{diff.size} bytes differ, first at {int(diff[0])} (element {int(diff[0]) // esz}: got " \
                  f"{got.view(np_dt)[int(diff[0]) // esz]!r}, want {want[int(diff[0]) // esz]!r}); " + why
        if (tail != 0xA5).any():
            why = f"{int((tail != 0xA5).sum())} guard bytes past the output written; " + why
        if why:
            bad.append(f"{tag}: {why}")
        else:
            n_ok += 1
    for b in bad:
        print(f"rank {rank} MISMATCH {b}", flush=True)
    print(f"rank {rank}: {n_ok} ok, {len(bad)} bad", flush=True)
    comm.destroy()
    dist.destroy_process_group()
    q.put((rank, n_ok, len(bad)))


if __name__ == "__main__":
    import multiprocessing as mp
    from tools._procs import join_ranks
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    mode = sys.argv[2] if len(sys.argv) > 2 else "small"
    rows = len(cases(P, mode))
    t0 = time.time()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(r, P, mode, 29657, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 240)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d mode=%s rows=%d wall=%.1fs" % (P, mode, rows, time.time() - t0), sorted(res), "exitcodes",
          [p.exitcode for p in ps], flush=True)
    sys.exit(0 if rows and len(res) == P and all(b == 0 and k == rows for _, k, b in res) else 1)
