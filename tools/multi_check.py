#!/usr/bin/env python3
"""Multi-buffer allreduce (bine_allreduce_multi) in real processes: P ranks share
the box's GPU, the seven-tensor list 5, 0, 1, 64, 8191, 3, 257 (each tensor one
element past a 16-B boundary), float SUM and bfloat16 wide "avg" (SUM times
1 / P), allreduce_bine_bdw_remap, out of place and in place, in three forms --
over RCCL point-to-point the literal and the flat schedule, and over the direct
peer-memory transport the flat one.  Every rank's tensors are compared with the
host statement of the single call on the concatenation: the oracle for float,
tests/wide_sim.py for the wide call; the bytes around every tensor must keep
their fill.
usage: python tools/multi_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = [5, 0, 1, 64, 8191, 3, 257]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
ROWS = (("float", "sum", False), ("bfloat16", "avg", True))
ALGO = "bine_bdw_remap"
CASES = len(FORMS) * len(ROWS) * 2


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
    total = sum(COUNTS)
    bad, n_ok = [], 0

    def arena(esz, data=None):
        """(device arena of 0xA5, its host image, the tensors' byte offsets)"""
        off, o = [], 0
        for c in COUNTS:
            off.append(o + 16 + esz)
            o = (o + 16 + esz + c * esz + 16 + 15) & ~15
        host = np.full(o + 16, 0xA5, dtype=np.uint8)
        if data is not None:
            raw, e = np.ascontiguousarray(data).view(np.uint8), 0
            for c, f in zip(COUNTS, off):
                host[f:f + c * esz] = raw[e:e + c * esz]
                e += c * esz
        return torch.from_numpy(host.copy()).to("cuda"), host, off

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    want = {}   # the host statement does not depend on the form
    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt, op, wide in ROWS:
            if dt not in want:
                if wide:
                    sb = H.inputs(dt, total, P, "sum")
                    want[dt] = (sb, WS.collective("allreduce", ALGO, sb, dt, "sum", None, True, 1.0 / P)[rank])
                else:
                    sb = O.inputs(dt, total, P)
                    want[dt] = (sb, O.allreduce(ALGO, sb, dt)[0][rank])
            sb, exp = want[dt]
            esz = sb[rank].dtype.itemsize
            for in_place in (False, True):
                ti, _, off = arena(esz, sb[rank])
                to, host, _ = (ti, None, None) if in_place else arena(esz)
                if in_place:
                    host = ti.cpu().numpy()
                rb = [to.data_ptr() + f for f in off]
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    pico_amd.allreduce_multi(ALGO, None if in_place else [ti.data_ptr() + f for f in off], rb, dt,
                                             op, comm, counts=COUNTS, wide=wide)
                torch.cuda.synchronize()
                comm.synchronize()
                got = to.cpu().numpy()
                mask = np.zeros(got.size, dtype=bool)
                for c, f in zip(COUNTS, off):
                    mask[f:f + c * esz] = True
                out = got[mask].view(sb[rank].dtype)
                ok = H.same(out, exp, dt) if wide else np.array_equal(out, exp)
                what = f"{form} {dt} {op} {'in place' if in_place else 'out of place'}"
                if not ok:
                    bad.append(f"{what}: {int((out != exp).sum())} elements differ")
                elif not np.array_equal(got[~mask], host[~mask]):
                    bad.append(f"{what}: bytes around a tensor changed")
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
    t0 = time.perf_counter()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=worker, args=(r, P, 29683, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
