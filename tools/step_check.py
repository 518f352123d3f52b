#!/usr/bin/env python3
"""Dynamic loss scaling in real processes: P ranks share the box's GPU, each
with the shards of seven tensors (0, 1, 5, 1023, 8192, 8193 and 40001 elements,
each one element past a 16-B boundary), float16 gradients stored as g * scale,
the float16 parameter tensors holding the current parameters, and a step state
in device memory.  In three forms -- over RCCL point-to-point the literal and
the flat schedule, and over the direct peer-memory transport the flat one --
two calls of norm_multi (bine_lat), step_update, adamw_multi_dyn (ring):
  taken: the state after the update against tests/step_sim.py on the norm the
    ranks agreed on, byte for byte, and equal on all ranks (exchanged over
    gloo); p', m', v' against tests/adamw_sim.py with the state's constants and
    multiplier, bit for bit; every rank's params the concatenation of all ranks'
    narrow(p'); g and the bytes around every tensor untouched;
  skipped: rank P - 1 alone holds one inf in one shard; every rank's state shows
    skip = 1, the scale halved, the step count as it was, the same bytes on all
    ranks; p, m, v and params keep every bit.
  graph mode (RCCL literal): the taken call twice on the same addresses with the
    same inputs -- step_update and k_adamw_segs stay ordinary launches, the
    inner collectives replay (graphs_cached() unchanged) and the bits are the same.
usage: python tools/step_check.py [P]   (exit 0 = every rank, every case ok)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = [0, 1, 5, 1023, 8192, 8193, 40001]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
DT = "float16"
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=1.0, clip_eps=1e-6,
             growth_interval=2000)
SCALE, STEP0 = 1024.0, 6
CASES = 2 * len(FORMS) + 1


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
    import step_sim as S
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    n = len(SHARDS)

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

    def gathered(x):
        every = [None] * P
        dist.all_gather_object(every, x)
        return every

    class Case:
        def __init__(self):
            rng = np.random.default_rng(100 * rank + 7)
            f32 = lambda c, s: (s * rng.standard_normal(c)).astype(np.float32)  # noqa: E731
            self.p = [f32(c, 1.0) for c in SHARDS]
            self.m = [f32(c, 0.1) for c in SHARDS]
            self.v = [f32(c, 0.1) ** 2 for c in SHARDS]
            # the stored gradient: g * scale, |g| around 1: far from float16's 65,504
            self.g = [H.from_f32(f32(c, 1.0) * np.float32(SCALE / 64), DT) for c in SHARDS]
            self.ar = {k: arena(SHARDS, 4, getattr(self, k)) for k in "pmv"}
            self.ar["g"] = arena(SHARDS, 2, self.g)
            mine = b"".join(A.narrow(x, DT).tobytes() for x in self.p)
            self.params0 = self.cat(gathered(mine))
            self.ar["params"] = arena([P * c for c in SHARDS], 2, [np.frombuffer(w, dtype=np.uint16)
                                                                   for w in self.params0])
            self.state0 = S.init(SCALE, STEP0, HYPER["beta1"], HYPER["beta2"])
            assert self.state0.tobytes() == pico_amd.step_state_init(SCALE, STEP0, HYPER["beta1"],
                                                                     HYPER["beta2"]).tobytes()
            self.state = torch.from_numpy(np.concatenate([np.full(16, 0xA5, dtype=np.uint8), self.state0,
                                                          np.full(16, 0xA5, dtype=np.uint8)])).to("cuda")
            self.stats = torch.zeros(n + 1, dtype=torch.float64, device="cuda")

        def cat(self, every):
            """tensor k: rank 0's shard, rank 1's, ..."""
            out, o = [], 0
            for c in SHARDS:
                out.append(b"".join(e[o:o + c * 2] for e in every))
                o += c * 2
            return out

        def ptrs(self, k):
            t, _, off = self.ar[k]
            return [t.data_ptr() + f for f in off]

        def reset(self):
            for k in ("p", "m", "v", "params"):
                t, host, _ = self.ar[k]
                t.copy_(torch.from_numpy(host))
            self.state[16:16 + S.BYTES].copy_(torch.from_numpy(self.state0))
            torch.cuda.synchronize()

        def plant_inf(self):
            t, host, off = self.ar["g"]
            host[off[5] + 2 * 77:off[5] + 2 * 77 + 2] = np.array([0x7C00], dtype=np.uint16).view(np.uint8)
            t.copy_(torch.from_numpy(host))

        def call(self):
            pico_amd.norm_multi("bine_lat", self.ptrs("g"), DT, comm, counts=SHARDS, stats=self.stats)
            pico_amd.step_update(self.state.data_ptr() + 16, self.stats.data_ptr() + 8 * n, **HYPER)
            pico_amd.adamw_multi_dyn("ring", self.ptrs("params"), self.ptrs("p"), self.ptrs("m"), self.ptrs("v"),
                                     self.ptrs("g"), self.state.data_ptr() + 16, comm, gdtype=DT, odtype=DT,
                                     shard_counts=SHARDS)

        def tensors(self, k):
            """(per tensor its bytes, whether the bytes around them are as they were)"""
            t, host, off = self.ar[k]
            got = t.cpu().numpy()
            esz = 4 if k in "pmv" else 2
            mask = np.zeros(got.size, dtype=bool)
            parts = []
            for c, f in zip([P * c for c in SHARDS] if k == "params" else SHARDS, off):
                mask[f:f + esz * c] = True
                parts.append(got[f:f + esz * c].tobytes())
            return parts, bool(np.array_equal(got[~mask], host[~mask]))

        def check(self, what, state_before, skipped):
            """None, or what differs; the state expected from state_before"""
            raw = self.state.cpu().numpy()
            st = raw[16:16 + S.BYTES]
            # the exchanges first, on every rank alike, whatever it then finds
            states = gathered(st.tobytes())
            f = S.fields(st)
            sim = [A.step(p, m, v, g, DT, f["consts"], np.float32(np.float64(f["gm"])))
                   for p, m, v, g in zip(self.p, self.m, self.v, self.g)]
            want_params = self.cat(gathered(b"".join(A.narrow(w[0], DT).tobytes() for w in sim)))
            if (raw[:16] != 0xA5).any() or (raw[16 + S.BYTES:] != 0xA5).any():
                return f"{what}: the bytes around the state changed"
            n2 = float(self.stats.cpu().numpy()[n])
            if skipped != (not n2 <= S.DBL_MAX):
                return f"{what}: the global norm is {n2}"
            want = S.update(state_before, n2, **HYPER)
            if st.tobytes() != want.tobytes():
                return f"{what}: the state differs from the sim: {S.fields(st)} against {S.fields(want)}"
            if len(set(states)) != 1:
                return f"{what}: the ranks' states differ"
            t, host, _ = self.ar["g"]
            if not np.array_equal(t.cpu().numpy(), host):
                return f"{what}: g or the bytes around it changed"
            if skipped:
                b = S.fields(state_before)
                if f["skip"] != 1.0 or f["scale"] != b["scale"] / 2 or f["step"] != b["step"]:
                    return f"{what}: a skipped state with {f}"
                for k in ("p", "m", "v", "params"):
                    if not np.array_equal(self.ar[k][0].cpu().numpy(), self.ar[k][1]):
                        return f"{what}: {k} changed on a skipped step"
                return None
            for j, k in enumerate("pmv"):
                parts, guards = self.tensors(k)
                if not guards:
                    return f"{what}: the bytes around {k} changed"
                for c, got, w in zip(SHARDS, parts, sim):
                    if got != w[j].tobytes():
                        return f"{what}: {k}' of a {c}-element shard differs from the sim"
            parts, guards = self.tensors("params")
            if not guards:
                return f"{what}: the bytes around params changed"
            if parts != want_params:
                return f"{what}: params differ from the ranks' narrow(p')"
            return None

        def keep(self):
            """what a skipped step must leave: the device's p, m, v, params become the host images"""
            for k in ("p", "m", "v", "params"):
                t, host, _ = self.ar[k]
                host[:] = t.cpu().numpy()
            return self.state.cpu().numpy()[16:16 + S.BYTES].copy()

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        c = Case()
        run(c.call)
        err = c.check(f"{form} taken", c.state0, False)
        bad.append(err) if err else None
        n_ok += not err
        after = c.keep()
        if rank == P - 1:
            c.plant_inf()
        run(c.call)
        err = c.check(f"{form} skipped", after, True)
        bad.append(err) if err else None
        n_ok += not err
    # graph mode: the second call on the same addresses replays the first one's graphs
    set_form(False, False)
    comm.set_graphs(True)
    c = Case()
    g0 = comm.graphs_cached()
    run(c.call)
    g1, e1 = comm.graphs_cached(), c.check("graphs first call", c.state0, False)
    first = [c.ar[k][0].cpu().numpy().copy() for k in ("p", "m", "v", "params")] + [c.state.cpu().numpy().copy()]
    c.reset()
    run(c.call)
    e2 = c.check("graphs second call", c.state0, False)
    second = [c.ar[k][0].cpu().numpy() for k in ("p", "m", "v", "params")] + [c.state.cpu().numpy()]
    if comm.graphs_cached() != g1 or g1 <= g0:
        bad.append(f"graphs: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
    elif e1 or e2:
        bad.append(e1 or e2)
    elif not all(np.array_equal(a, b) for a, b in zip(first, second)):
        bad.append("graphs: the replay's bits differ")
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
    ps = [ctx.Process(target=worker, args=(r, P, 29696, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
