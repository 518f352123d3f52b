#!/usr/bin/env python3
"""Global norm and clipping (bine_norm_multi / bine_clip_multi) in real processes:
P ranks share the box's GPU, each with seven tensors whose counts differ from
rank to rank (0, 1, 5, 1023, 1024, 8193, 40000 plus the rank's number, each
tensor one element past a 16-B boundary), in three forms -- over RCCL
point-to-point the literal and the flat schedule, and over the direct
peer-memory transport the flat one -- for float and bfloat16, bine_lat:
  norm_multi: every rank's stats against the host statement: the oracle's
    allreduce (double, sum) of the vectors bine_sumsq_segments wrote on the ranks
    (exchanged over gloo), bit for bit; those vectors against math.fsum of the
    exact squares within counts[k] * 2^-52;
  clip_multi: stats[0..n] as norm_multi's, stats[n + 1] = numpy float64's
    min(1, max_norm / (sqrt(stats[n]) + eps)) bit for bit and the same on every
    rank, every tensor = bine_scale by that coefficient, the bytes around the
    tensors untouched; before it clip_multi(scale=False): the same statistics
    and coefficient, the tensors and the bytes around them untouched;
  graph mode (RCCL literal): norm_multi twice on the same buffers -- the second
    call replays (graphs_cached() unchanged) and gives the same bits.
usage: python tools/norm_check.py [P]   (exit 0 = every rank, every case ok)
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = [0, 1, 5, 1023, 1024, 8193, 40000]
FORMS = (("rccl literal", False, False), ("rccl flat", False, True), ("direct flat", True, True))
TYPES = ("float", "bfloat16")
ALGO = "bine_lat"
MAX_NORM, EPS = 5.0, 1e-6
CASES = len(FORMS) * len(TYPES) * 3 + 1


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
    from oracle import oracle as O
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    comm = pico_amd.Comm.from_torch_distributed(dev)
    side = torch.cuda.Stream()
    bad, n_ok = [], 0
    counts = [c + rank if c else 0 for c in BASE]
    n = len(counts)

    def arena(dt):
        """(device arena of 0xA5 with the tensors in it, its host image, byte offsets, the values as float64)"""
        esz = 4 if dt == "float" else 2
        rng = np.random.default_rng(100 * rank + esz)
        off, o, vals = [], 0, []
        for c in counts:
            off.append(o + 16 + esz)
            o = (o + 16 + esz + c * esz + 16 + 15) & ~15
        host = np.full(o + 16, 0xA5, dtype=np.uint8)
        for c, f in zip(counts, off):
            x = rng.standard_normal(c).astype(np.float32)
            st = x if dt == "float" else H.from_f32(x, dt)
            host[f:f + c * esz] = st.view(np.uint8)
            vals.append((x if dt == "float" else H.to_f32(st, dt)).astype(np.float64))
        return torch.from_numpy(host.copy()).to("cuda"), host, off, vals, esz

    def set_form(direct, flat):
        comm.set_direct(direct)
        comm.set_flat_rs(flat)
        comm.set_flat_ag(2 if flat else 0)
        comm.set_chunk(4096 if flat else 0)

    def local_vector(dt, t, off, vals):
        """what bine_sumsq_segments writes here, checked against the exact sums"""
        ptrs = [t.data_ptr() + f for f in off]
        v = pico_amd.sumsq_segments(ptrs, dt, counts=counts)
        torch.cuda.synchronize()
        v = v.cpu().numpy()
        for k, c in enumerate(counts):
            exact = math.fsum((vals[k] * vals[k]).tolist())
            if abs(v[k] - exact) > c * 2.0 ** -52 * exact:
                bad.append(f"{dt} sumsq tensor {k}: {v[k]!r} for {exact!r}")
        return v

    def host_statement(v):
        """the oracle's allreduce of every rank's vector"""
        vs = [None] * P
        dist.all_gather_object(vs, v.tobytes())
        want, _ = O.allreduce(ALGO, [np.frombuffer(b, dtype=np.float64).copy() for b in vs], "double")
        return np.ascontiguousarray(want[rank])

    def coef(norm2):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float64(MAX_NORM) / (np.sqrt(np.float64(norm2)) + np.float64(EPS))
        return r if r < 1.0 else np.float64(1.0)

    def run(fn):
        with torch.cuda.stream(side):
            fn()
        torch.cuda.synchronize()
        comm.synchronize()

    for form, direct, flat in FORMS:
        set_form(direct, flat)
        for dt in TYPES:
            t, host, off, vals, esz = arena(dt)
            ptrs = [t.data_ptr() + f for f in off]
            want = host_statement(local_vector(dt, t, off, vals))
            stats = torch.full((n + 1,), -1.0, dtype=torch.float64, device="cuda")
            run(lambda: pico_amd.norm_multi(ALGO, ptrs, dt, comm, counts=counts, stats=stats))
            got = stats.cpu().numpy()
            if got.tobytes() != want.tobytes():
                bad.append(f"{form} norm_multi {dt}: {got[-1]!r} for {want[-1]!r}")
            elif not np.array_equal(t.cpu().numpy(), host):
                bad.append(f"{form} norm_multi {dt}: the tensors or the bytes around them changed")
            else:
                n_ok += 1
            c = coef(want[n])
            # the coefficient alone: clip_multi(scale=False) leaves the tensors as they are
            stats0 = torch.full((n + 2,), -1.0, dtype=torch.float64, device="cuda")
            run(lambda: pico_amd.clip_multi(ALGO, ptrs, dt, comm, MAX_NORM, EPS, counts=counts, stats=stats0,
                                            scale=False))
            got = stats0.cpu().numpy()
            what = f"{form} clip_multi(scale=False) {dt}"
            if got[:n + 1].tobytes() != want.tobytes() or got[n + 1].tobytes() != c.tobytes():
                bad.append(f"{what}: stats or coefficient {got[n + 1]!r} for {c!r}")
            elif not np.array_equal(t.cpu().numpy(), host):
                bad.append(f"{what}: the tensors or the bytes around them changed")
            else:
                n_ok += 1
            # clip_multi on the same tensors; the reference: bine_scale per tensor on a copy
            ref = t.clone()
            for cnt, f in zip(counts, off):
                if cnt:
                    pico_amd.scale(ref.data_ptr() + f, ref.data_ptr() + f, cnt, dt, scale=float(c))
            stats2 = torch.full((n + 2,), -1.0, dtype=torch.float64, device="cuda")
            run(lambda: pico_amd.clip_multi(ALGO, ptrs, dt, comm, MAX_NORM, EPS, counts=counts, stats=stats2))
            got = stats2.cpu().numpy()
            cs = [None] * P
            dist.all_gather_object(cs, got[n + 1].tobytes())
            what = f"{form} clip_multi {dt}"
            if got[:n + 1].tobytes() != want.tobytes():
                bad.append(f"{what}: stats differ from norm_multi's")
            elif got[n + 1].tobytes() != c.tobytes() or len(set(cs)) != 1 or not c < 1.0:
                bad.append(f"{what}: coefficient {got[n + 1]!r} for {c!r}, {len(set(cs))} values over the ranks")
            elif not torch.equal(t, ref):
                bad.append(f"{what}: {int((t != ref).sum())} bytes differ from bine_scale's")
            else:
                n_ok += 1
    # graph mode: the second call on the same buffers replays the first one's graph
    set_form(False, False)
    comm.set_graphs(True)
    t, host, off, vals, esz = arena("float")
    ptrs = [t.data_ptr() + f for f in off]
    stats = torch.full((n + 1,), -1.0, dtype=torch.float64, device="cuda")
    g0 = comm.graphs_cached()
    run(lambda: pico_amd.norm_multi(ALGO, ptrs, "float", comm, counts=counts, stats=stats))
    g1, first = comm.graphs_cached(), stats.cpu().numpy().copy()
    stats.fill_(-1.0)
    run(lambda: pico_amd.norm_multi(ALGO, ptrs, "float", comm, counts=counts, stats=stats))
    second = stats.cpu().numpy()
    want = host_statement(local_vector("float", t, off, vals))
    if comm.graphs_cached() != g1 or g1 <= g0:
        bad.append(f"graphs norm_multi: {g0} -> {g1} -> {comm.graphs_cached()} cached graphs")
    elif first.tobytes() != want.tobytes() or second.tobytes() != want.tobytes():
        bad.append("graphs norm_multi: the bits differ from the host statement")
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
    ps = [ctx.Process(target=worker, args=(r, P, 29688, q)) for r in range(P)]
    for p in ps:
        p.start()
    join_ranks(ps, 150)   # the ranks' own time limit: stragglers are stopped
    res = [q.get() for _ in range(sum(1 for p in ps if p.exitcode == 0))]
    print("RESULT P=%d" % P, sorted(res), "exitcodes", [p.exitcode for p in ps],
          "wall %.1f s" % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if len(res) == P and all(b == 0 and k == CASES for _, k, b in res) else 1)
