#!/usr/bin/env python3
"""Wide (binary32-accumulating) allreduce / reduce-scatter in real processes: P
ranks share the box's GPU, float16 and bfloat16, SUM with scale 1/P and MAX
with scale 1, allreduce_bine_bdw_remap and reduce_scatter_bine_permute_remap at
2 * 4099 and 4 * 2048 elements, in three forms -- over RCCL point-to-point the
literal schedule (path A: k_widen, the binary32 call, k_narrow) and the flat
one (path B: the 16-bit plan with BINE_PRIM_WIDE trees), and over the direct
peer-memory transport the flat one (path B: pull copies plus the wide tree as
a separate launch).  Every case runs a second time under BINE_WIDE_TREES=0
(path A everywhere; over the direct transport the binary32 call then takes the
transport's in-launch float trees, fused into one launch where the blocks are
multiples of 16 B: the 4 * 2048 count).  Every rank's output of both runs is
compared with the host statement of the definition (tests/wide_sim.py).
usage: python tools/wide_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (2 * 4099, 4 * 2048)
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = ("float16", "bfloat16")
OPS = (("sum", None), ("max", 1.0))   # scale None: 1 / P
COLLS = (("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_permute_remap"))
CASES = 2 * len(COUNTS) * len(FORMS) * len(TYPES) * len(OPS) * len(COLLS)


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
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0

    def call(coll, algo, s, r, n, rc, dt, op, scale):
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            if coll == "allreduce":
                pico_amd.allreduce_wide(algo, s, r, n, dt, op, comm, scale=scale)
            else:
                pico_amd.reduce_scatter_wide(algo, s, r, rc, dt, op, comm, scale=scale)
        torch.cuda.synchronize()
        comm.synchronize()

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    want = {}   # the host statement does not depend on the form: computed once per case
    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for n in COUNTS:
            for dt in TYPES:
                for op, scale in OPS:
                    scale = 1.0 / P if scale is None else scale
                    for coll, algo in COLLS:
                        rc = [n // P] * P if coll == "reduce_scatter" else None
                        key = (n, dt, op, coll)
                        if key not in want:
                            sb = H.inputs(dt, sum(rc) if rc else n, P, op)
                            want[key] = (sb, WS.collective(coll, algo, sb, dt, op, rc, False, scale)[rank])
                        sb, exp = want[key]
                        path_b = pico_amd.wide_plan(coll, algo, P, count=n, rcounts=rc, flat_ag=2 if flat else 0,
                                                    flat_rs=flat)
                        if path_b != flat:
                            bad.append(f"{form} {coll} n={n}: wide_plan says {'B' if path_b else 'A'}")
                        s = torch.from_numpy(sb[rank].view(np.uint8).copy()).to("cuda")
                        for forced_a in (False, True):
                            if forced_a:
                                os.environ["BINE_WIDE_TREES"] = "0"
                            else:
                                os.environ.pop("BINE_WIDE_TREES", None)
                            r = torch.full((exp.size * 2,), 0xA5, dtype=torch.uint8, device="cuda")
                            call(coll, algo, s, r, n, rc, dt, op, scale)
                            got = r.cpu().numpy().view(np.uint16)
                            if H.same(got, exp, dt):
                                n_ok += 1
                            else:
                                bad.append(f"{form} {coll} {algo} {dt} {op} n={n} "
                                           f"{'path A forced' if forced_a else 'default path'}: "
                                           f"{int((got != exp).sum())} elements differ")
    os.environ.pop("BINE_WIDE_TREES", None)
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
    ps = [ctx.Process(target=worker, args=(r, P, 29671, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
