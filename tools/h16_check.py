#!/usr/bin/env python3
"""float16 / bfloat16 collectives in real processes: P ranks share the box's
GPU, SUM with allreduce_bine_bdw_remap and reduce_scatter_bine_permute_remap
(count 2 * 4099) in three forms -- over RCCL point-to-point the literal
schedule and the flat one, and over the direct peer-memory transport the flat
one, where these types take the pull copies + k_reduce_tree path (the
transport's in-launch tree kernels are not provided for them).  Every rank's
output is compared with the host replay of the literal plan under the 16-bit
arithmetic of tests/h16_util.py.
usage: python tools/h16_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2 * 4099
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))


def worker(rank, P, port, q):
    from tools._procs import rank_device
    dev = rank_device(rank)   # (sets the fake RCCL host id on the one-GPU box)
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    import numpy as np
    import pico_amd
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import h16_util as H
    import plan_sim
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    for form, direct, flat in FORMS:
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)
        for dt in H.TYPES:
            for coll, algo in (("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_permute_remap")):
                rc = [N // P] * P if coll == "reduce_scatter" else None
                sb = H.inputs(dt, N, P, "sum")
                with H.patched():
                    want = plan_sim.run(coll, algo, [x.copy() for x in sb], dt, "sum", rcounts=rc)[rank]
                s = torch.from_numpy(sb[rank].view(np.uint8).copy()).to("cuda")
                r = torch.full((want.size * 2,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    if coll == "allreduce":
                        pico_amd.allreduce(algo, s, r, N, dt, "sum", comm)
                    else:
                        pico_amd.reduce_scatter(algo, s, r, rc, dt, "sum", comm)
                torch.cuda.synchronize()
                comm.synchronize()
                got = r.cpu().numpy().view(np.uint16)
                if H.same(got, want, dt):
                    n_ok += 1
                else:
                    bad.append(f"{form} {coll} {algo} {dt}: {int((got != want).sum())} elements differ")
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
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(r, P, 29641, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 120)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps], flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == 12 for _, k, b in res) else 1)
