#!/usr/bin/env python3
"""Fused AdamW step and allgather (bine_adamw_multi) in real processes: P ranks
share the box's GPU, each with the shards of seven tensors (0, 1, 5, 1023, 8192,
8193 and 40001 elements, each one element past a 16-B boundary) and the full
parameter tensors, in three forms -- over RCCL point-to-point the literal and
the flat schedule, and over the direct peer-memory transport the flat one -- for
float (g and params float) and bfloat16 (g and params bfloat16), ring:
  adamw_multi: this rank's p', m', v' against tests/adamw_sim.py, the numpy
    float32 statement, bit for bit; every rank's params against the
    concatenation of all ranks' narrow(p') (exchanged over gloo), bit for bit;
    g and the bytes around every tensor untouched; gcoef read from the device;
  graph mode (RCCL literal): the call twice on the same addresses with the same
    inputs -- the second call replays (graphs_cached() unchanged) and gives the
    same bits.
usage: python tools/adamw_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = [0, 1, 5, 1023, 8192, 8193, 40001]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = ("float", "bfloat16")
ALGO = "ring"
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=7)
GCOEF, GRAD_MUL = 0.37, 1.0 / 1024
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
    import adamw_sim as A
    import h16_util as H
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    n = len(SHARDS)
    coef = torch.tensor([GCOEF], dtype=torch.float64, device="cuda")
    gm = A.gm_of(GCOEF, GRAD_MUL)

    def arena(counts, esz, data):
        """(device arena of 0xA5 with the tensors in it, its host image, byte offsets)"""
        off, o = [], 0
        for c in counts:
            off.append(o + 16 + esz)
            o = (o + 16 + esz + c * esz + 16 + 15) & ~15
        host = np.full(o + 16, 0xA5, dtype=np.uint8)
        for c, f, x in zip(counts, off, data):
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
        def __init__(self, dt):
            self.dt, self.esz = dt, 4 if dt == "float" else 2
            rng = np.random.default_rng(100 * rank + self.esz)
            f32 = lambda c, s: (s * rng.standard_normal(c)).astype(np.float32)  # noqa: E731
            self.p = [f32(c, 1.0) for c in SHARDS]
            self.m = [f32(c, 0.1) for c in SHARDS]
            self.v = [f32(c, 0.1) ** 2 for c in SHARDS]
            self.g = [f32(c, 1.0) if dt == "float" else H.from_f32(f32(c, 1.0), dt) for c in SHARDS]
            self.ar = {k: arena(SHARDS, 4, getattr(self, k)) for k in "pmv"}
            self.ar["g"] = arena(SHARDS, self.esz, self.g)
            fill = np.float32 if dt == "float" else np.uint16
            self.ar["params"] = arena([P * c for c in SHARDS], self.esz, [np.full(P * c, 7, dtype=fill) for c in SHARDS])
            consts = pico_amd.adamw_consts(**HYPER)
            self.want = [A.step(p, m, v, g, dt, consts, gm) for p, m, v, g in zip(self.p, self.m, self.v, self.g)]
            mine = b"".join(A.narrow(w[0], dt).tobytes() for w in self.want)
            every = [None] * P
            dist.all_gather_object(every, mine)
            self.params_want = []
            o = 0
            for c in SHARDS:     # tensor k: rank 0's shard, rank 1's, ...
                self.params_want.append(b"".join(e[o:o + c * self.esz] for e in every))
                o += c * self.esz

        def ptrs(self, k):
            t, _, off = self.ar[k]
            return [t.data_ptr() + f for f in off]

        def reset(self):
            for k in "pmv":
                t, host, _ = self.ar[k]
                t.copy_(torch.from_numpy(host))
            torch.cuda.synchronize()

        def call(self):
            pico_amd.adamw_multi(ALGO, self.ptrs("params"), self.ptrs("p"), self.ptrs("m"), self.ptrs("v"),
                                 self.ptrs("g"), comm, gcoef=coef, grad_mul=GRAD_MUL, gdtype=self.dt, odtype=self.dt,
                                 shard_counts=SHARDS, **HYPER)

        def check(self, what):
            """None, or what differs"""
            for j, k in enumerate("pmv"):
                t, host, off = self.ar[k]
                got = t.cpu().numpy()
                mask = np.zeros(got.size, dtype=bool)
                for c, f, w in zip(SHARDS, off, self.want):
                    mask[f:f + 4 * c] = True
                    if got[f:f + 4 * c].tobytes() != w[j].tobytes():
                        return f"{what}: {k}' of a {c}-element shard differs from the sim"
                if not np.array_equal(got[~mask], host[~mask]):
                    return f"{what}: the bytes around {k} changed"
            t, host, off = self.ar["params"]
            got = t.cpu().numpy()
            mask = np.zeros(got.size, dtype=bool)
            for c, f, w in zip(SHARDS, off, self.params_want):
                mask[f:f + len(w)] = True
                if got[f:f + len(w)].tobytes() != w:
                    return f"{what}: params of the {c}-element shards differ from the ranks' narrow(p')"
            if not np.array_equal(got[~mask], host[~mask]):
                return f"{what}: the bytes around params changed"
            t, host, _ = self.ar["g"]
            if not np.array_equal(t.cpu().numpy(), host):
                return f"{what}: g or the bytes around it changed"
            return None

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt in TYPES:
            c = Case(dt)
            run(c.call)
            err = c.check(f"{form} adamw_multi {dt}")
            if err:
                bad.append(err)
            else:
                n_ok += 1
    # graph mode: the second call on the same addresses replays the first one's graph
    set_form(False, False)
    comm.set_graphs(True)
    c = Case("bfloat16")
    g0 = comm.graphs_cached()
    run(c.call)
    g1, e1 = comm.graphs_cached(), c.check("graphs first call")
    first = c.ar["params"][0].cpu().numpy().copy()
    c.reset()
    c.ar["params"][0].copy_(torch.from_numpy(c.ar["params"][1]))
    run(c.call)
    e2 = c.check("graphs second call")
    if comm.graphs_cached() != g1 or g1 <= g0:
        bad.append(f"graphs adamw_multi: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
    elif e1 or e2:
        bad.append(e1 or e2)
    elif not np.array_equal(first, c.ar["params"][0].cpu().numpy()):
        bad.append("graphs adamw_multi: the replay's bits differ")
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
    ps = [ctx.Process(target=worker, args=(r, P, 29694, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
