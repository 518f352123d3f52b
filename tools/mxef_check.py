#!/usr/bin/env python3
"""MX-quantized gradient reduce-scatter with an error-feedback residual
(bine_mx_reduce_scatter_multi_ef) in real processes: P ranks share the box's
GPU, each with the gradients of six tensors (P shards of 0, 32, 64, 8192, 8224
and 40000 elements, each one element past a 16-B boundary), a float32 residual
per gradient and two workspaces of P wire blocks, in three forms -- over RCCL
point-to-point the literal and the flat schedule, and over the direct
peer-memory transport the flat one -- for float gradients through e4m3 and
bfloat16 gradients through e2m1:
  mx_reduce_scatter_multi_ef twice, the second call carrying the residuals the
    first one left: every rank's shards and residuals against
    tests/mxef_sim.py over all ranks' gradients and residuals (exchanged over
    gloo), bit for bit; the sources and the bytes around every tensor, residual
    and workspace untouched;
  graph mode (RCCL literal): the same two calls on the same addresses -- the
    all-to-all of the second call replays (graphs_cached() unchanged) and both
    calls give the sim's bytes.
usage: python tools/mxef_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = [0, 32, 64, 8192, 8224, 40000]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = (("float", "e4m3", "sum"), ("bfloat16", "e2m1", "avg"))
CASES = len(FORMS) * len(TYPES) + 1


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
    import fp8_sim as F
    import h16_util as H
    import mxef_sim as E
    import mxrs_sim as R
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    n = len(SHARDS)

    def arena(counts, esz, phase, data):
        """(device arena of 0xA5 with the tensors in it, its host image, byte offsets)"""
        off, o = [], 0
        for k, c in enumerate(counts):
            off.append(o + 16 + phase(k))
            o = (o + 16 + phase(k) + c * esz + 16 + 15) & ~15
        host = np.full(o + 16, 0xA5, dtype=np.uint8)
        for c, f, x in zip(counts, off, data):
            if x is not None:
                host[f:f + c * esz] = np.ascontiguousarray(x).view(np.uint8)
        return torch.from_numpy(host.copy()).to("cuda"), host, off

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    def run(fn):
        with torch.cuda.stream(side):
            fn()
        torch.cuda.synchronize()
        comm.synchronize()

    class Case:
        def __init__(self, dt, fmt, op):
            self.dt, self.fmt, self.op, self.esz = dt, fmt, op, 4 if dt == "float" else 2
            rng = np.random.default_rng(100 * rank + self.esz)
            self.x, self.r = [], []
            for c in SHARDS:
                top = np.repeat(rng.integers(-20, 20, P * c // 32), 32)
                x = (rng.standard_normal(P * c) * np.exp2(top - rng.integers(0, 12, P * c))).astype(np.float32)
                x = x if dt == "float" else H.from_f32(x, dt)
                self.x.append(x)
                self.r.append((F.widen(x, dt) * (rng.standard_normal(P * c) * 0.1).astype(np.float32)).astype(np.float32))
            self.B = R.layout(SHARDS, fmt)[3]
            self.src = arena([P * c for c in SHARDS], self.esz, lambda k: self.esz, self.x)
            self.res = arena([P * c for c in SHARDS], 4, lambda k: 4 * (k % 2), self.r)     # both bodies
            self.dst = arena(SHARDS, self.esz, lambda k: self.esz * (k % 2), [None] * n)
            self.sws = arena([P * self.B], 1, lambda k: 0, [None])
            self.rws = arena([P * self.B], 1, lambda k: 0, [None])
            every = [None] * P
            dist.all_gather_object(every, ([x.tobytes() for x in self.x], [r.tobytes() for r in self.r]))
            view = np.float32 if dt == "float" else np.uint16
            grads = [[np.frombuffer(b, dtype=view) for b in e[0]] for e in every]
            res = [[np.frombuffer(b, dtype=np.float32) for b in e[1]] for e in every]
            scale = 1.0 / P if op == "avg" else 1.0
            self.want = []                       # per call (this rank's shards, this rank's residuals)
            for _ in range(2):
                out, res, _ = E.reduce_scatter_ef(grads, res, SHARDS, dt, dt, fmt, scale)
                self.want.append((out[rank], res[rank]))

        def ptrs(self, ar):
            t, _, off = ar
            return [t.data_ptr() + f for f in off]

        def call(self):
            pico_amd.mx_reduce_scatter_multi_ef(self.ptrs(self.src), self.ptrs(self.res), self.ptrs(self.dst), self.fmt,
                                                comm, op=self.op, sdtype=self.dt, rdtype=self.dt, shard_counts=SHARDS,
                                                send_ws=self.ptrs(self.sws)[0], recv_ws=self.ptrs(self.rws)[0])

        def check(self, what, call):
            """None, or what differs after call 0 or 1"""
            shards, resid = self.want[call]
            t, host, off = self.dst
            got = t.cpu().numpy()
            mask = np.zeros(got.size, dtype=bool)
            for k, (c, f) in enumerate(zip(SHARDS, off)):
                mask[f:f + c * self.esz] = True
                if R.same(got[f:f + c * self.esz].view(R.VIEW[self.dt]), shards[k], self.dt).size:
                    return f"{what}: the {c}-element shard differs from the sim"
            if not np.array_equal(got[~mask], host[~mask]):
                return f"{what}: the bytes around the shards changed"
            t, host, off = self.res
            got = t.cpu().numpy()
            mask = np.zeros(got.size, dtype=bool)
            for k, (c, f) in enumerate(zip(SHARDS, off)):
                mask[f:f + P * c * 4] = True
                if not np.array_equal(got[f:f + P * c * 4].view(np.uint32), resid[k].view(np.uint32)):
                    return f"{what}: the residual of the {c}-element shards differs from the sim"
            if not np.array_equal(got[~mask], host[~mask]):
                return f"{what}: the bytes around the residuals changed"
            for name, (t, host, off) in (("send_ws", self.sws), ("recv_ws", self.rws)):
                got = t.cpu().numpy()
                mask = np.zeros(got.size, dtype=bool)
                mask[off[0]:off[0] + P * self.B] = True
                if not np.array_equal(got[~mask], host[~mask]):
                    return f"{what}: the bytes around {name} changed"
            t, host, _ = self.src
            if not np.array_equal(t.cpu().numpy(), host):
                return f"{what}: the sources or the bytes around them changed"
            return None

        def two_calls(self, what):
            for i in range(2):
                run(self.call)
                err = self.check(f"{what} call {i + 1}", i)
                if err:
                    return err
            return None

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt, fmt, op in TYPES:
            err = Case(dt, fmt, op).two_calls(f"{form} mx_reduce_scatter_multi_ef {dt} {fmt}")
            if err:
                bad.append(err)
            else:
                n_ok += 1
    # graph mode: the second call on the same addresses replays the first one's graphs
    set_form(False, False)
    comm.set_graphs(True)
    c = Case("float", "e4m3", "sum")
    g0 = comm.graphs_cached()
    run(c.call)
    g1, e1 = comm.graphs_cached(), c.check("graphs first call", 0)
    run(c.call)
    e2 = c.check("graphs second call", 1)
    if comm.graphs_cached() != g1 or g1 <= g0:
        bad.append(f"graphs mx_reduce_scatter_multi_ef: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
    elif e1 or e2:
        bad.append(e1 or e2)
    else:
        n_ok += 1
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
    ps = [ctx.Process(target=worker, args=(r, P, 29695, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
