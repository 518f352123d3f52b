#!/usr/bin/env python3
"""MX block-scaled parameter allgather (bine_mx_quant_multi) in real processes:
P ranks share the box's GPU, each with the shards of six tensors (0, 32, 64,
8192, 8224 and 40000 elements, each one element past a 16-B boundary) and the
full tensors' data and scale bytes at odd byte phases, in three forms -- over
RCCL point-to-point the literal and the flat schedule, and over the direct
peer-memory transport the flat one -- for float sources to e4m3 and bfloat16
sources to e2m1, ring for the allgather:
  mx_quant_multi: every rank's params8 and scales8 against tests/mx_sim.py's
    two steps over all ranks' shards (exchanged over gloo), bit for bit; the
    sources and the bytes around every tensor untouched;
  graph mode (RCCL literal): the call twice on the same addresses with the same
    inputs -- the second call replays (graphs_cached() unchanged) and gives the
    same bytes.
usage: python tools/mx_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = [0, 32, 64, 8192, 8224, 40000]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = (("float", "e4m3"), ("bfloat16", "e2m1"))
AG_ALGO = "ring"
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
    import h16_util as H
    import mx_sim as M
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
        def __init__(self, dt, fmt):
            self.dt, self.fmt, self.esz = dt, fmt, 4 if dt == "float" else 2
            rng = np.random.default_rng(100 * rank + self.esz)
            self.x = []
            for c in SHARDS:
                top = np.repeat(rng.integers(-60, 60, (c + 31) // 32), 32)[:c]
                x = (rng.standard_normal(c) * np.exp2(top - rng.integers(0, 12, c))).astype(np.float32)
                self.x.append(x if dt == "float" else H.from_f32(x, dt))
            self.src = arena(SHARDS, self.esz, lambda k: self.esz, self.x)
            self.p8 = arena([P * M.dbytes(c, fmt) for c in SHARDS], 1, lambda k: (3 * k + 1) % 8, [None] * n)
            self.s8 = arena([P * (c // 32) for c in SHARDS], 1, lambda k: (k + 1) % 4, [None] * n)
            every = [None] * P
            dist.all_gather_object(every, [x.tobytes() for x in self.x])
            view = np.float32 if dt == "float" else np.uint16
            shards = [[np.frombuffer(b, dtype=view) for b in e] for e in every]
            self.want8, self.wants = M.quant_multi(shards, dt, fmt)

        def ptrs(self, ar):
            t, _, off = ar
            return [t.data_ptr() + f for f in off]

        def reset(self):
            self.p8[0].copy_(torch.from_numpy(self.p8[1]))
            self.s8[0].copy_(torch.from_numpy(self.s8[1]))
            torch.cuda.synchronize()

        def call(self):
            pico_amd.mx_quant_multi(AG_ALGO, self.ptrs(self.p8), self.ptrs(self.s8), self.ptrs(self.src), self.fmt,
                                    comm, sdtype=self.dt, shard_counts=SHARDS)

        def check(self, what):
            """None, or what differs"""
            for name, ar, want in (("params8", self.p8, self.want8), ("scales8", self.s8, self.wants)):
                t, host, off = ar
                got = t.cpu().numpy()
                mask = np.zeros(got.size, dtype=bool)
                for c, f, w in zip(SHARDS, off, want):
                    mask[f:f + w.size] = True
                    if not np.array_equal(got[f:f + w.size], w):
                        return f"{what}: {name} of the {c}-element shards differ from the sim"
                if not np.array_equal(got[~mask], host[~mask]):
                    return f"{what}: the bytes around {name} changed"
            t, host, _ = self.src
            if not np.array_equal(t.cpu().numpy(), host):
                return f"{what}: the sources or the bytes around them changed"
            return None

        def state(self):
            return self.p8[0].cpu().numpy().tobytes() + self.s8[0].cpu().numpy().tobytes()

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt, fmt in TYPES:
            c = Case(dt, fmt)
            run(c.call)
            err = c.check(f"{form} mx_quant_multi {dt} {fmt}")
            if err:
                bad.append(err)
            else:
                n_ok += 1
    # graph mode: the second call on the same addresses replays the first one's graphs
    set_form(False, False)
    comm.set_graphs(True)
    c = Case("float", "e4m3")
    g0 = comm.graphs_cached()
    run(c.call)
    g1, e1 = comm.graphs_cached(), c.check("graphs first call")
    first = c.state()
    c.reset()
    run(c.call)
    e2 = c.check("graphs second call")
    if comm.graphs_cached() != g1 or g1 <= g0:
        bad.append(f"graphs mx_quant_multi: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
    elif e1 or e2:
        bad.append(e1 or e2)
    elif first != c.state():
        bad.append("graphs mx_quant_multi: the replay's bytes differ")
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
    ps = [ctx.Process(target=worker, args=(r, P, 29699, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
