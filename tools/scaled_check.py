#!/usr/bin/env python3
"""Scaled allreduce / reduce-scatter in real processes: P ranks share the box's
GPU, SUM with scale 1/3, allreduce_bine_bdw_remap and
reduce_scatter_bine_permute_remap (count 2 * 4099), fp32 and bf16, in three
forms -- over RCCL point-to-point the literal schedule (a trailing k_scale)
and the flat one (the flagged trees scale), and over the direct peer-memory
transport the flat one: for fp32 the transport's in-launch trees followed by
one k_scale over the output, for bf16 pull copies plus the scaled tree.  One
more case runs the RCCL flat form in graph mode: twice with scale 1/3 and once
with scale 3.0 on the same buffers, every result checked (the scale is part of
the graph's key).  Every rank's output is compared with S(host replay of the
literal unscaled plan) (tests/scale_sim.py).
usage: python tools/scaled_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2 * 4099
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = ("float", "bfloat16")
COLLS = (("allreduce", "bine_bdw_remap"), ("reduce_scatter", "bine_permute_remap"))
CASES = len(FORMS) * len(TYPES) * len(COLLS) + 3


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
    import scale_sim as SS
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0

    def host_inputs(dt):
        if dt in H.TYPES:
            return H.inputs(dt, N, P, "sum")
        return [(np.random.default_rng(1234 + r).random(N) * 100.0).astype(np.float32) for r in range(P)]

    def same(got, want, dt):
        if dt in H.TYPES:
            return H.same(got, want, dt)
        return got.tobytes() == want.tobytes()

    def call(coll, algo, s, r, rc, dt, scale):
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            if coll == "allreduce":
                pico_amd.allreduce(algo, s, r, N, dt, "sum", comm, scale=scale)
            else:
                pico_amd.reduce_scatter(algo, s, r, rc, dt, "sum", comm, scale=scale)
        torch.cuda.synchronize()
        comm.synchronize()

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt in TYPES:
            nd = SS.np_dtype(dt)
            for coll, algo in COLLS:
                rc = [N // P] * P if coll == "reduce_scatter" else None
                sb = host_inputs(dt)
                lit = SS.run(coll, algo, sb, dt, "sum", rcounts=rc)[rank]
                want = SS.S(lit, dt, 1 / 3)
                s = torch.from_numpy(sb[rank].view(np.uint8).copy()).to("cuda")
                r = torch.full((want.size * want.dtype.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
                call(coll, algo, s, r, rc, dt, 1 / 3)
                got = r.cpu().numpy().view(nd)
                if same(got, want, dt):
                    n_ok += 1
                else:
                    bad.append(f"{form} {coll} {algo} {dt}: {int((got != want).sum())} elements differ")
    # graph mode, RCCL flat: the same buffers with two different scales
    set_form(False, True)
    comm.set_graphs(True)
    sb = host_inputs("float")
    lit = SS.run("allreduce", "bine_bdw_remap", sb, "float", "sum")[rank]
    s = torch.from_numpy(sb[rank].view(np.uint8).copy()).to("cuda")
    r = torch.full((N * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    for k, scale in enumerate((1 / 3, 1 / 3, 3.0)):
        r.fill_(0xA5)
        call("allreduce", "bine_bdw_remap", s, r, None, "float", scale)
        got = r.cpu().numpy().view(np.float32)
        if same(got, SS.S(lit, "float", scale), "float"):
            n_ok += 1
        else:
            bad.append(f"graph mode call {k} scale {scale}: {int((got != SS.S(lit, 'float', scale)).sum())} differ")
    cached = comm.graphs_cached()
    if cached == 0:
        print(f"rank {rank}: graph mode kept the calls eager on this runtime: the key was not exercised", flush=True)
    else:
        print(f"rank {rank}: {cached} graphs cached (two scales, two graphs)", flush=True)
        if cached != 2:
            bad.append(f"graph mode: {cached} graphs cached for two scales")
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
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(r, P, 29643, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 120)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps], flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
