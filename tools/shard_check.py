#!/usr/bin/env python3
"""Sharded multi-buffer reduce-scatter and allgather (bine_reduce_scatter_multi /
bine_allgather_multi) in real processes: P ranks share the box's GPU, the
seven-tensor list of shard counts 0, 1, 5, 1023, 1024, 8193, 40000 (each tensor
one element past a 16-B boundary), in three forms -- over RCCL point-to-point
the literal and the flat schedule, and over the direct peer-memory transport the
flat one.
  reduce-scatter (bine_permute_remap): float SUM and bfloat16 wide "avg" (SUM
    times 1 / P), out of place and with rbufs[k] the head of sbufs[k]; every rank
    against the host statement of the single call on the rank-major packed buffer
    (the oracle for float, tests/wide_sim.py for the wide call);
  allgather (ring): float and bfloat16, out of place and in place (sbufs=None);
    every rank against the concatenation of the ranks' inputs;
  graph mode (RCCL literal): each collective twice on the same buffers -- the
    second call replays (graphs_cached() unchanged) and gives the same bits.
The bytes around every tensor must keep their fill.
usage: python tools/shard_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = [0, 1, 5, 1023, 1024, 8193, 40000]
B = sum(COUNTS)
OFF = [sum(COUNTS[:k]) for k in range(len(COUNTS))]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
RS_ROWS = (("float", "sum", False), ("bfloat16", "avg", True))
AG_TYPES = ("float", "bfloat16")
RS_ALGO, AG_ALGO = "bine_permute_remap", "ring"
CASES = len(FORMS) * (len(RS_ROWS) * 2 + len(AG_TYPES) * 2) + 2


def worker(rank, P, port, q):
    from tools._procs import rank_device
    dev = rank_device(rank)   # (sets the fake RCCL host id on the one-GPU box)
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    os.environ.pop("BINE_WIDE_TREES", None)
    import numpy as np
    import pico_amd
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import h16_util as H
    import wide_sim as WS
    from oracle import oracle as O
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0

    def arena(counts, esz, parts=None):
        """(device arena of 0xA5, its host image, the tensors' byte offsets)"""
        off, o = [], 0
        for c in counts:
            off.append(o + 16 + esz)
            o = (o + 16 + esz + c * esz + 16 + 15) & ~15
        host = np.full(o + 16, 0xA5, dtype=np.uint8)
        if parts is not None:
            for c, f, x in zip(counts, off, parts):
                host[f:f + c * esz] = np.ascontiguousarray(x).view(np.uint8)
        return torch.from_numpy(host.copy()).to("cuda"), host, off

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    def judge(what, t, host, off, counts, esz, exp, same):
        """the tensors of arena t (counts[k] elements at off[k]) against exp, the rest against host"""
        nonlocal n_ok
        got = t.cpu().numpy()
        mask = np.zeros(got.size, dtype=bool)
        for c, f in zip(counts, off):
            mask[f:f + c * esz] = True
        out = got[mask].view(exp.dtype)
        if not same(out, exp):
            bad.append(f"{what}: {int((out != exp).sum())} elements differ, first {out[:2]} for {exp[:2]}")
        elif not np.array_equal(got[~mask], host[~mask]):
            bad.append(f"{what}: bytes around a tensor changed")
        else:
            n_ok += 1
        return out

    def flat_of(M, k):
        return np.concatenate([M[j * B + OFF[k]:j * B + OFF[k] + COUNTS[k]] for j in range(P)])

    full = [P * c for c in COUNTS]
    rs_want, ag_in = {}, {}   # the host statements do not depend on the form
    for dt, op, wide in RS_ROWS:
        if wide:
            Ms = H.inputs(dt, P * B, P, "sum")
            exp = WS.collective("reduce_scatter", RS_ALGO, Ms, dt, "sum", [B] * P, False, 1.0 / P)[rank][:B]
        else:
            Ms = O.inputs(dt, P * B, P)
            exp = O.reduce_scatter(RS_ALGO, Ms, [B] * P, dt)[0][rank]
        rs_want[dt] = (Ms[rank], np.ascontiguousarray(exp))
    for dt in AG_TYPES:
        xs = O.inputs(dt, B, P) if dt == "float" else H.inputs(dt, B, P)
        ag_in[dt] = (xs, np.concatenate([np.concatenate([x[o:o + c] for x in xs]) for o, c in zip(OFF, COUNTS)]))

    def rs_call(dt, op, wide, alias):
        M, exp = rs_want[dt]
        esz = M.dtype.itemsize
        ti, hi, ioff = arena(full, esz, [flat_of(M, k) for k in range(len(COUNTS))])
        to, ho, off = (ti, hi, ioff) if alias else arena(COUNTS, esz)
        sb = [ti.data_ptr() + f for f in ioff]
        rb = [to.data_ptr() + f for f in off]
        assert all(f + c * esz + 16 <= to.numel() for f, c in zip(off, COUNTS))
        torch.cuda.synchronize()

        def call(keep=(ti, to)):   # the arenas live as long as the call does
            with torch.cuda.stream(side):
                pico_amd.reduce_scatter_multi(RS_ALGO, sb, rb, dt, op, comm, shard_counts=COUNTS, wide=wide)
            torch.cuda.synchronize()
            comm.synchronize()
        same = (lambda a, b: H.same(a, b, dt)) if wide else np.array_equal
        return call, (lambda what: judge(what, to, ho, off, COUNTS, esz, exp, same))

    def ag_call(dt, in_place):
        xs, exp = ag_in[dt]
        esz = xs[rank].dtype.itemsize
        mine = [xs[rank][o:o + c] for o, c in zip(OFF, COUNTS)]
        to, ho, off = arena(full, esz)
        if in_place:
            for c, f, x in zip(COUNTS, off, mine):
                ho[f + rank * c * esz:f + (rank + 1) * c * esz] = np.ascontiguousarray(x).view(np.uint8)
            to.copy_(torch.from_numpy(ho))
            ti, sb = None, None
        else:
            ti, _, ioff = arena(COUNTS, esz, mine)
            sb = [ti.data_ptr() + f for f in ioff]
        rb = [to.data_ptr() + f for f in off]
        torch.cuda.synchronize()

        def call(keep=(ti, to)):
            with torch.cuda.stream(side):
                pico_amd.allgather_multi(AG_ALGO, sb, rb, dt, comm, shard_counts=COUNTS)
            torch.cuda.synchronize()
            comm.synchronize()
        return call, (lambda what: judge(what, to, ho, off, full, esz, exp, np.array_equal))

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt, op, wide in RS_ROWS:
            for alias in (False, True):
                call, check = rs_call(dt, op, wide, alias)
                call()
                check(f"{form} reduce_scatter {dt} {op} {'rbufs in sbufs' if alias else 'out of place'}")
        for dt in AG_TYPES:
            for in_place in (False, True):
                call, check = ag_call(dt, in_place)
                call()
                check(f"{form} allgather {dt} {'in place' if in_place else 'out of place'}")
    # graph mode: the second call on the same buffers replays the first one's graph
    set_form(False, False)
    comm.set_graphs(True)
    for name, (call, check) in (("reduce_scatter", rs_call("float", "sum", False, False)),
                                ("allgather", ag_call("float", False))):
        ok0, bad0, g0 = n_ok, len(bad), comm.graphs_cached()
        call()
        g1 = comm.graphs_cached()
        first = check(f"graphs {name} first call").copy()
        call()
        second = check(f"graphs {name} second call")
        if comm.graphs_cached() != g1 or g1 <= g0:
            bad.append(f"graphs {name}: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
        elif not np.array_equal(first.view(np.uint8), second.view(np.uint8)):
            bad.append(f"graphs {name}: the replay's bits differ")
        n_ok = ok0 + (len(bad) == bad0)   # one case: both calls right, one graph, replayed
    comm.set_graphs(False)
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
    t0 = time.perf_counter()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(r, P, 29684, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
